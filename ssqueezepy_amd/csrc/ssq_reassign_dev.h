// ssq_reassign_dev.h -- device-side pieces shared by the reassignment kernels: the additive term of a point (Term; the
// accumulate kernels of ssq_kernels.hip and the three column-tile kernels), the ordered combine of the lanes of a DPP
// row (dpp_mov, FoldLower; accumulate_tile16_kernel, conceft_kernel, time_reassign_kernel) and the 16-byte point types
// of the streaming maps (Phase2Vec, phase2_abs; the second-order phase kernels, time_reassign_kernel).
#pragma once
#include "ssq_common.h"

namespace ssq {

template <int CTRL> __device__ __forceinline__ int dpp_mov(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL> __device__ __forceinline__ float dpp_mov(float old, float v) {
    return __int_as_float(dpp_mov<CTRL>(__float_as_int(old), __float_as_int(v)));
}
template <int CTRL> __device__ __forceinline__ double dpp_mov(double old, double v) {
    int lo = dpp_mov<CTRL>(__double2loint(old), __double2loint(v));
    int hi = dpp_mov<CTRL>(__double2hiint(old), __double2hiint(v));
    return __hiloint2double(hi, lo);
}

// the additive term of one point and how it is folded into a cell, in the CPU path's
// arithmetic: float32 data with a float64 weight vector accumulates through double (algos.py:66-79)
template <typename T, bool CST64> struct Term {
    using type = T;
    using wtype = T;
    static __device__ __forceinline__ T make(T z, T w) { return z * w; }
    static __device__ __forceinline__ T fold(T o, T t) { return o + t; }
};
template <> struct Term<float, true> {
    using type = double;
    using wtype = double;
    static __device__ __forceinline__ double make(float z, double w) { return (double)z * w; }
    static __device__ __forceinline__ float fold(float o, double t) { return (float)((double)o + t); }
};

// fold in the terms of row-lanes rl-15 .. rl-1 that target the same cell, ascending.
// The match test of distance N yields a wave mask (one compare); from it come, for
// free on the scalar unit, (a) the decision whether anything has to move at this
// distance and (b) the "a higher row-lane hits my cell" mask: lane L+N matching at
// distance N is lane L having a higher partner at distance N (row_shr never crosses a
// 16-lane row, so mask >> N stays inside the column).
// SC (scalar combine): the per-distance decision is one DPP move + one compare, the rest
// scalar -- measured faster with 8 row-lanes (245 vs 263 us), slower with 16 (263 vs 257),
// so each layout keeps the form that suits it.
// A step around it is: read the target cell, FoldLower, add the lane's own term, the highest lane of a key stores.
// Those lines stay written out in the three kernels: as one inline function (cell pointer and term handed over, or
// made inside) the compiler hoists the address and the term out of the branch of the lanes that take part, or orders
// the step's loads differently, in at least two of the three -- profiles/reassign_fold_isa.txt.
template <int N, bool SC, typename TM, typename T, typename term_t>
struct FoldLower {
    static __device__ __forceinline__ void run(int k, unsigned long long valid, term_t tr, term_t ti,
                                               T& ore, T& oim, unsigned long long& higher) {
        // row_shr:N with bound_ctrl: lanes without a source in their row read 0. Keys are
        // bin + 1 (0 = "takes no part", `valid` = the wave mask of k != 0), so a lane that
        // takes part never matches a missing source.
        const int ks = __builtin_amdgcn_update_dpp(0, k, 0x110 + N, 0xF, 0xF, true);
        bool m;
        unsigned long long mask;
        if constexpr (SC) {
            const bool e = ks == k;
            mask = __builtin_amdgcn_ballot_w64(e) & valid;
            m = e & (k != 0);
        } else {
            m = (ks == k) & (k != 0);
            mask = __ballot(m);
        }
        if (mask) {                                         // wave-uniform
            higher |= mask >> N;
            term_t rs = dpp_mov<0x110 + N>(term_t(0), tr), is = dpp_mov<0x110 + N>(term_t(0), ti);
            if (m) { ore = TM::fold(ore, rs); oim = TM::fold(oim, is); }
        }
        FoldLower<N - 1, SC, TM, T, term_t>::run(k, valid, tr, ti, ore, oim, higher);
    }
};
template <bool SC, typename TM, typename T, typename term_t>
struct FoldLower<0, SC, TM, T, term_t> {
    static __device__ __forceinline__ void run(int, unsigned long long, term_t, term_t, T&, T&,
                                               unsigned long long&) {}
};

// 16 bytes of a complex plane: two float32 points or one float64 point
typedef float phase2_f4v __attribute__((ext_vector_type(4)));
typedef float phase2_f2v __attribute__((ext_vector_type(2)));
typedef double phase2_d2v __attribute__((ext_vector_type(2)));
template <typename T> struct Phase2Vec;
template <> struct Phase2Vec<float> { using load_t = phase2_f4v; using store_t = phase2_f2v; static constexpr int PTS = 2; };
template <> struct Phase2Vec<double> { using load_t = phase2_d2v; using store_t = double; static constexpr int PTS = 1; };

__device__ __forceinline__ double phase2_abs(double x, double y, float) { return sqrt(x * x + y * y); }   // (float32 data: the squares cannot leave float64's range)
__device__ __forceinline__ double phase2_abs(double x, double y, double) { return hypot(x, y); }

}  // namespace ssq
