// ssq_time_reassign.hip -- ssq_time_reassign: the time-reassigned synchrosqueezing transform (TSST; He, Cao, Zi, Zhou,
// Chen 2019) -- every coefficient of a (batch, rows, n) plane moves along its row to its local group delay. Kernel,
// launcher and C-ABI entries. include/ssq_hip.h states what is computed; DESIGN.md section 4.5.7 the sizing. Compiled
// with -ffp-contract=off, like ssq_kernels.hip, whose ordered row-lane combine and 16-byte point types it shares
// (ssq_reassign_dev.h).
//
// A wavefront (a workgroup of 64) owns the destination cells [c0, c0 + TSSQ_SEG) of one row of one signal as an LDS
// strip of float64 complex cells. It walks the sources [c0 - dmax, c0 + len + dmax) in ascending blocks of 64 -- lane =
// source column, so the loads are coalesced; the next block's two points and its rotation are requested before the
// current block is used -- and keeps the terms that land in its own strip. A cell's terms must be added in ascending
// source order. Blocks are in order because one wavefront issues them. Within a block every lane first writes its
// lane number to its cell's byte of a tag array and reads it back: if every lane finds its own, no two terms of the
// block share a cell and each lane adds its term to its cell directly (the common case: a tone moves nothing, noise
// scatters). Otherwise the four 16-lane DPP rows take their turn one after the other, and inside a row FoldLower
// gives every lane cell + the terms of the lower lanes with its key, ascending, and the highest lane of a key
// stores: any pattern of keys, adjacent or not, is added in lane order (an impulse sends all 64 to one cell).
// Which lane's tag survives a clash does not matter: only "all found their own" is used. Nothing is shared between
// wavefronts, so there are no atomics and the result does not depend on the grid; the strip leaves in full lines,
// rounded once.
#include "ssq_common.h"
#include "ssq_reassign_dev.h"
#include <cfloat>
#include <type_traits>

namespace ssq {

constexpr int TSSQ_SEG = 960;                   // cells of a strip: 15 KiB of LDS + 960 tag bytes, ten strips per CU
constexpr int64_t TSSQ_MAX_DMAX = 1 << 20;      // keeps a displacement and a wavefront's walk (SEG + 2 dmax) in 32 bits
constexpr int64_t TSSQ_MAX_GRID = 1 << 24;      // workgroups of a launch; a workgroup takes units grid-stride

template <typename T, bool VEC>
__global__ __launch_bounds__(64) void time_reassign_kernel(
    const T* __restrict__ Sx, const T* __restrict__ Vtg, const double* __restrict__ rot, T* __restrict__ Tx,
    int64_t units, unsigned rows, unsigned n, unsigned segs, unsigned n_fft, unsigned hop_m, double cps, int dmax,
    double gamma) {
    using TM = Term<double, false>;
    using load_t = std::conditional_t<sizeof(T) == 4, phase2_f2v, phase2_d2v>;      // one complex point
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* strip = reinterpret_cast<double*>(lds_raw);
    unsigned char* tag = lds_raw + (size_t)(n < TSSQ_SEG ? n : TSSQ_SEG) * 16;      // a byte per cell, after the strip
    const int lane = threadIdx.x;

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const unsigned row = (unsigned)(unit / segs), seg = (unsigned)(unit - (int64_t)row * segs);   // row = b * rows + i
        const unsigned i = row % rows;
        const int64_t c0 = (int64_t)seg * TSSQ_SEG;
        const int len = (int)((int64_t)n - c0 < TSSQ_SEG ? (int64_t)n - c0 : TSSQ_SEG);
        const size_t roff = (size_t)row * (size_t)n;             // (the host guarantees batch rows n < 2^32)
        for (int t = lane; t < 2 * len; t += 64) strip[t] = 0.0;
        __builtin_amdgcn_wave_barrier();

        const int64_t lo = c0 - dmax > 0 ? c0 - dmax : 0;
        const int64_t hi = c0 + len + dmax < (int64_t)n ? c0 + len + dmax : (int64_t)n;
        // p = (i c hop) mod n_fft, exact: a = i hop mod n_fft (i < n_fft < 2^31), p(c) = a (c mod n_fft) mod n_fft
        // for a lane's first column and p(c + 64) = p(c) + 64 a mod n_fft from then on
        const unsigned a = (unsigned)(((uint64_t)i * hop_m) % n_fft), a64 = (unsigned)((64ull * a) % n_fft);
        int64_t c = lo + lane;
        unsigned p = (unsigned)(((uint64_t)a * ((uint64_t)c % n_fft)) % n_fft);

        // loads are unconditional (the column clamped, the point discarded at its use)
        auto load = [&](int64_t col, unsigned pp, T& gr, T& gi, T& tr, T& ti, double& ur, double& ui) {
            const size_t o = roff + (size_t)(col < hi ? col : hi - 1);
            if constexpr (VEC) {
                const load_t g = reinterpret_cast<const load_t*>(Sx)[o], t = reinterpret_cast<const load_t*>(Vtg)[o];
                gr = g.x; gi = g.y; tr = t.x; ti = t.y;
            } else {
                gr = Sx[2 * o]; gi = Sx[2 * o + 1]; tr = Vtg[2 * o]; ti = Vtg[2 * o + 1];
            }
            if (rot) { ur = rot[2 * (size_t)pp]; ui = rot[2 * (size_t)pp + 1]; }
            else { ur = 1.0; ui = 0.0; }
        };
        T ngr, ngi, ntr, nti;
        double nur, nui;
        load(c, p, ngr, ngi, ntr, nti, nur, nui);
        for (int64_t base = lo; base < hi; base += 64) {
            const double gr = (double)ngr, gi = (double)ngi, tr = (double)ntr, ti = (double)nti, ur = nur, ui = nui;
            const unsigned pn = p >= n_fft - a64 ? p - (n_fft - a64) : p + a64;
            if (base + 64 < hi) load(c + 64, pn, ngr, ngi, ntr, nti, nur, nui);

            int key = 0;                                        // cell + 1; 0: the point takes no part
            double vr = 0.0, vi = 0.0;
            if (c < hi && !(phase2_abs(gr, gi, T(0)) < gamma)) {
                const double s = (tr * gr + ti * gi) / (gr * gr + gi * gi);
                const double d = rint(s * cps);
                if (fabs(d) <= (double)dmax) {                  // (false for NaN)
                    const int64_t c2 = c + (int64_t)(int)d;
                    if (c2 >= c0 && c2 < c0 + len) {
                        key = (int)(c2 - c0) + 1;
                        vr = ur * gr - ui * gi; vi = ur * gi + ui * gr;
                    }
                }
            }
            const unsigned long long valid = __builtin_amdgcn_ballot_w64(key != 0);
            if (valid) {                                                        // (wave-uniform, as all below)
                // (the byte must really go to LDS and come back -- another lane may have overwritten it. wave_barrier
                // orders the schedule only; the memory clobber keeps the compiler from forwarding the stored value)
                if (key) tag[key - 1] = (unsigned char)lane;
                __builtin_amdgcn_wave_barrier();
                asm volatile("" ::: "memory");
                const bool clash = key && tag[key - 1] != (unsigned char)lane;
                if (!__builtin_amdgcn_ballot_w64(clash)) {                      // every term has a cell of its own
                    if (key) {
                        double* cell = strip + 2 * (key - 1);
                        cell[0] = cell[0] + vr; cell[1] = cell[1] + vi;
                    }
                    __builtin_amdgcn_wave_barrier();
                } else {
                    for (int r = 0; r < 4; ++r) {
                        if (!((valid >> (16 * r)) & 0xFFFFull)) continue;
                        const int kr = (lane >> 4) == r ? key : 0;
                        double ore = 0.0, oim = 0.0;
                        double* cell = strip;
                        if (kr) { cell = strip + 2 * (kr - 1); ore = cell[0]; oim = cell[1]; }
                        unsigned long long higher = 0;
                        FoldLower<15, false, TM, double, double>::run(kr, valid, vr, vi, ore, oim, higher);
                        ore = ore + vr; oim = oim + vi;
                        if (kr && !((higher >> lane) & 1ull)) { cell[0] = ore; cell[1] = oim; }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
            c += 64; p = pn;
        }

        for (int t = lane; t < len; t += 64) {
            const size_t o = roff + (size_t)(c0 + t);
            if constexpr (VEC) {
                load_t v;
                v.x = (T)strip[2 * t]; v.y = (T)strip[2 * t + 1];
                reinterpret_cast<load_t*>(Tx)[o] = v;
            } else {
                Tx[2 * o] = (T)strip[2 * t]; Tx[2 * o + 1] = (T)strip[2 * t + 1];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <typename T>
static int launch_time_reassign(const void* Sx, const void* Vtg, const void* rot, void* Tx, int64_t batch, int64_t rows,
                                int64_t n, int64_t n_fft, int64_t hop_len, double cps, int64_t dmax, double gamma,
                                hipStream_t stream) {
    const int64_t segs = (n + TSSQ_SEG - 1) / TSSQ_SEG, units = batch * rows * segs;
    const size_t lds = (size_t)(n < TSSQ_SEG ? n : TSSQ_SEG) * 17;          // a cell and its tag byte
    // one load per point needs every plane on a 16-byte boundary (a caller's offset pointer need not be)
    const bool vec = (uintptr_t)Sx % 16 == 0 && (uintptr_t)Vtg % 16 == 0 && (uintptr_t)Tx % 16 == 0;
    return launch_lds(vec ? time_reassign_kernel<T, true> : time_reassign_kernel<T, false>,
                      dim3((unsigned)(units < TSSQ_MAX_GRID ? units : TSSQ_MAX_GRID)), dim3(64), lds, stream, (const T*)Sx,
                      (const T*)Vtg, (const double*)rot, (T*)Tx, units, (unsigned)rows, (unsigned)n, (unsigned)segs,
                      (unsigned)n_fft, (unsigned)(hop_len % n_fft), cps, (int)dmax, gamma);
}

}  // namespace ssq

using namespace ssq;

extern "C" {

int ssq_time_reassign_segment(void) { return TSSQ_SEG; }
int ssq_time_reassign_max_dmax(void) { return (int)TSSQ_MAX_DMAX; }

int ssq_time_reassign(int dtype, const void* Sx, const void* Vtg, const void* rot, void* Tx, int64_t batch, int64_t rows,
                      int64_t n, int64_t n_fft, int64_t hop_len, double cols_per_second, int64_t dmax, double gamma,
                      void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Sx && Vtg && Tx, "ssq_time_reassign: null pointer");
    SSQ_REQUIRE(batch >= 1 && rows >= 1 && n >= 1, "ssq_time_reassign: bad shape (%lld, %lld, %lld): batch, rows, n >= 1",
                (long long)batch, (long long)rows, (long long)n);
    if (check_point_count("ssq_time_reassign", batch, rows, n)) return -1;
    SSQ_REQUIRE(n_fft >= 1 && n_fft <= (int64_t)0x7FFFFFFF && hop_len >= 1,
                "ssq_time_reassign: n_fft = %lld, hop_len = %lld: n_fft 1 .. 2^31 - 1, hop_len >= 1", (long long)n_fft,
                (long long)hop_len);
    SSQ_REQUIRE(rows <= n_fft, "ssq_time_reassign: %lld rows of an n_fft of %lld", (long long)rows, (long long)n_fft);
    SSQ_REQUIRE(dmax >= 0 && dmax <= TSSQ_MAX_DMAX, "ssq_time_reassign: dmax = %lld, 0 .. %lld", (long long)dmax,
                (long long)TSSQ_MAX_DMAX);
    SSQ_REQUIRE(cols_per_second > 0.0 && cols_per_second <= DBL_MAX,
                "ssq_time_reassign: cols_per_second must be positive and finite (got %g)", cols_per_second);
    if (check_gamma("ssq_time_reassign", gamma)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_time_reassign<T>(Sx, Vtg, rot, Tx, batch, rows, n, n_fft, hop_len, cols_per_second, dmax, gamma,
                                       as_stream(stream));
    });
}

}  // extern "C"

// The fixed-point scatter (peak, windowed 64-bit integer scatter, finish: one kernel skeleton, one launcher) shares this
// unit's flags and point types; its three rules and their entries follow it:
#include "ssq_fixed_scatter.inl"
// ssq_reassign2d, the reassigned spectrogram: the energy moves along both axes at once
#include "ssq_reassign2d.inl"
// ssq_reassign_cwt, the reassigned scalogram: the CWT form, rows to bins of the synchrosqueezing grid
#include "ssq_reassign_cwt.inl"
// ssq_time_reassign_cwt, the time-reassigned synchrosqueezed CWT: signed complex terms, two words per cell
#include "ssq_time_reassign_cwt.inl"
