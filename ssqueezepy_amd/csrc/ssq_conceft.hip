// ssq_conceft.hip -- ssq_conceft, ssq_conceft_cwt: multitaper synchrosqueezing (ConceFT; Daubechies, Wang, Wu 2016) in
// one kernel, in its STFT and its CWT form: kernel, projection table, launcher and the two C-ABI entries.
// include/ssq_hip.h states what is computed; DESIGN.md section 4.5.5 the sizing. Compiled with -ffp-contract=off (bin
// indices), like ssq_kernels.hip, whose ordered row-lane combine it shares (ssq_reassign_dev.h).
//
// A workgroup owns a tile of TC adjacent columns of one signal, a wavefront WC = 4 of them x 16 row-lanes (lane =
// 16 * column + row-lane) -- the float64 layout of accumulate_tile16_kernel. Its wavefronts never synchronise with each
// other: each has its own slab of the LDS tile (rows x 4 complex128 cells, skewed like the tile kernel's), and
// keeps the running sums of the cells k = row-lane + 16 s of its own columns in registers (NC of them per lane).
// Per projection q: the point's J pairs (V_j, dV_j) are loaded (after the first projection they come from the
// caches: a tile's planes are J * rows * TC * 32 bytes at most), mixed in float64 with r[q][.] -- which sits in scalar
// registers, read through the constant address space --, thresholded, mapped to a bin by the exact map and added to
// the tile in ascending row order; then every lane folds its cells into its sums and clears them.
// HBM traffic: the 2J planes once, Cx once; nothing of size (Q, rows, n) exists anywhere.
// CWT = false is ssq_conceft: a row's value is Sfs[i] (the planes' real dtype), w = |Sfs[i] - phase_ratio| and a term is
// Vq. CWT = true is ssq_conceft_cwt: a row's value is the weight cst[i] (float64), w = |phase_ratio| and a term is
// Vq * cst[i]; on the log grids the bin map takes log2(w), inside the branch that a point below gamma skips.
#include "ssq_common.h"
#include "ssq_reassign_dev.h"
#include <type_traits>

namespace ssq {

#include "ssq_point_math.inl"

struct ConceftPlanes { const void* v[8]; const void* dv[8]; };

// rows a tile of TC columns supports: TC * 16 bytes per row in 160 KiB of LDS, 16 NC cells per column in registers
constexpr int64_t CONCEFT_MAX_ROWS = 1280;

template <typename T, int TC, int NC, bool CPLX, bool CWT>
__global__ __launch_bounds__(64 * (TC / 4)) void conceft_kernel(
    ConceftPlanes P, const std::conditional_t<CWT, double, T>* __restrict__ Sfs, const double* __restrict__ proj,
    T* __restrict__ Cx, SsqParams sp, int J, int Q, int rows, int n, unsigned tiles) {
    constexpr int RL = 16, WC = 4;
    using TM = Term<double, false>;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cl = lane / RL, rl = lane % RL;
    const unsigned b = blockIdx.x / tiles, tile_id = blockIdx.x - b * tiles;
    if ((int64_t)tile_id * TC + wave * WC >= n) return;        // (wave-uniform: the wavefront has no column)
    const int j = (int)tile_id * TC + wave * WC + cl;
    const bool col_ok = j < n;
    const int jc = col_ok ? j : n - 1;
    const int64_t omax = rows - 1;
    const size_t boff = (size_t)b * (size_t)rows * (size_t)n;   // (the host guarantees batch rows n < 2^32)
    double* slab = reinterpret_cast<double*>(lds_raw) + (size_t)wave * rows * WC * 2;
    const auto* r = SSQ_CONST_PTR(double, proj);

    for (int t = lane; t < rows * WC * 2; t += 64) slab[t] = 0.0;
    double acc[NC][CPLX ? 2 : 1];
#pragma unroll
    for (int s = 0; s < NC; ++s) { acc[s][0] = 0.0; if constexpr (CPLX) acc[s][1] = 0.0; }
    __builtin_amdgcn_wave_barrier();

    for (int q = 0; q < Q; ++q) {
        const auto* rq = r + 2 * (size_t)q * J;
        for (int i0 = 0; i0 < rows; i0 += RL) {
            const int i = i0 + rl;
            const int ic = i < rows ? i : rows - 1;
            // loads are unconditional (row and column clamped, the point discarded at its use) and all 2J of a
            // point are requested before the first is used
            const size_t off = boff + (size_t)((unsigned)ic * (unsigned)n + (unsigned)jc);
            T zr[8], zi[8], er[8], ei[8];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t < J) {
                    const T* z = (const T*)P.v[t] + 2 * off;
                    const T* e = (const T*)P.dv[t] + 2 * off;
                    zr[t] = z[0]; zi[t] = z[1]; er[t] = e[0]; ei[t] = e[1];
                }
            const double sf = (double)Sfs[ic];
            double vr = 0.0, vi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t < J) {
                    const double ar = rq[2 * t], ai = rq[2 * t + 1];
                    vr = vr + (ar * (double)zr[t] - ai * (double)zi[t]);
                    vi = vi + (ar * (double)zi[t] + ai * (double)zr[t]);
                    dr = dr + (ar * (double)er[t] - ai * (double)ei[t]);
                    di = di + (ar * (double)ei[t] + ai * (double)er[t]);
                }
            int k = -1;
            if (col_ok && i < rows && !(hypot(vr, vi) < sp.gamma)) {
                if constexpr (CWT) k = (int)bin_from_w(fabs(phase_ratio(dr, di, vr, vi)), sp, omax);
                else k = (int)bin_from_w(fabs(sf - phase_ratio(dr, di, vr, vi)), sp, omax);
                if (sp.flipud) k = (int)omax - k;
            }
            // the 16 rows of the step, combined in registers in ascending row order: one LDS read and one LDS write
            // per cell and step (accumulate_tile16_kernel)
            double tr = 0.0, ti = 0.0, ore = 0.0, oim = 0.0;
            double* cell = slab;
            if (k >= 0) {
                if constexpr (CWT) { tr = vr * sf; ti = vi * sf; }
                else { tr = vr; ti = vi; }
                cell = slab + 2 * (k * WC + ((cl + k) & (WC - 1)));
                ore = cell[0]; oim = cell[1];
            }
            unsigned long long higher = 0;
            const int key = k + 1;
            FoldLower<RL - 1, false, TM, double, double>::run(key, __builtin_amdgcn_ballot_w64(key != 0), tr, ti, ore, oim,
                                                              higher);
            ore = ore + tr; oim = oim + ti;
            if (k >= 0 && !((higher >> lane) & 1ull)) { cell[0] = ore; cell[1] = oim; }
            __builtin_amdgcn_wave_barrier();
        }
        // fold T_q into the running sums and clear it. An empty cell is skipped: it would add +0.
#pragma unroll
        for (int s = 0; s < NC; ++s) {
            const int k = rl + RL * s;
            if (k < rows) {
                double* cell = slab + 2 * (k * WC + ((cl + k) & (WC - 1)));
                const double re = cell[0], im = cell[1];
                if (re != 0.0 || im != 0.0) {
                    if constexpr (CPLX) { acc[s][0] = acc[s][0] + re; acc[s][1] = acc[s][1] + im; }
                    else acc[s][0] = acc[s][0] + hypot(re, im);
                    cell[0] = 0.0; cell[1] = 0.0;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (!col_ok) return;
    const double qd = (double)Q;
#pragma unroll
    for (int s = 0; s < NC; ++s) {
        const int k = rl + RL * s;
        if (k < rows) {
            const size_t o = boff + (size_t)((unsigned)k * (unsigned)n + (unsigned)j);
            if constexpr (CPLX) { Cx[2 * o] = (T)(acc[s][0] / qd); Cx[2 * o + 1] = (T)(acc[s][1] / qd); }
            else Cx[o] = (T)(acc[s][0] / qd);
        }
    }
}

// r[q][j] on the current device, (Q, J, 2) float64: uploaded once per (device, contents) and kept
static DeviceTableCache g_conceft_tables;

template <typename T, bool CPLX, bool CWT>
static int launch_conceft(const ConceftPlanes& P, const void* Sfs, const double* proj, void* Cx, const SsqParams& sp,
                          int64_t batch, int64_t J, int64_t Q, int64_t rows, int64_t n, hipStream_t stream) {
    using R = std::conditional_t<CWT, double, T>;             // the row vector's element: Sfs, or the float64 weights
    // the widest tile whose rows fit the LDS and whose cells fit the lanes' registers
    auto launch = [&](auto tc, auto nc) -> int {
        constexpr int TC = decltype(tc)::value, NC = decltype(nc)::value;
        const unsigned tiles = (unsigned)((n + TC - 1) / TC);
        return launch_lds(conceft_kernel<T, TC, NC, CPLX, CWT>, dim3(tiles * (unsigned)batch), dim3(64 * (TC / 4)),
                          (size_t)rows * TC * 16, stream, P, (const R*)Sfs, proj, (T*)Cx, sp, (int)J, (int)Q, (int)rows,
                          (int)n, tiles);
    };
    if (rows <= 16 * 17) return launch(int_c<16>{}, int_c<17>{});
    if (rows <= 16 * 40) return launch(int_c<16>{}, int_c<40>{});
    return launch(int_c<8>{}, int_c<80>{});
}

}  // namespace ssq

using namespace ssq;

// ssq_conceft and ssq_conceft_cwt: one set of checks, one launcher. `rowv` is Sfs (the planes' real dtype) for the STFT
// form and the float64 weights cst for the CWT form; `name` opens every refusal's message.
static int conceft_entry(bool cwt, const char* name, int dtype, const void* const* V, const void* const* dV,
                         const void* rowv, const double* proj, void* Cx, int64_t batch, int64_t J, int64_t Q, int64_t rows,
                         int64_t n, double gamma, int grid, const double* params, int flipud, int average, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(J >= 1 && J <= 8, "%s: J = %lld, 1 .. 8 transforms", name, (long long)J);
    SSQ_REQUIRE(Q >= 1 && Q <= 1024, "%s: Q = %lld, 1 .. 1024 projections", name, (long long)Q);
    SSQ_REQUIRE(batch >= 1 && rows >= 2 && n >= 1, "%s: bad shape (%lld, %lld, %lld): rows >= 2, batch, n >= 1", name,
                (long long)batch, (long long)rows, (long long)n);
    SSQ_REQUIRE(rows <= CONCEFT_MAX_ROWS, "%s: %lld rows, at most %lld (an 8-column float64 tile in 160 KiB of LDS)", name,
                (long long)rows, (long long)CONCEFT_MAX_ROWS);
    if (check_point_count(name, batch, rows, n)) return -1;
    SSQ_REQUIRE(V && dV && rowv && proj && Cx && params, "%s: null pointer", name);
    ConceftPlanes P = {};
    for (int64_t j = 0; j < J; ++j) {
        SSQ_REQUIRE(V[j] && dV[j], "%s: plane %lld is a null pointer", name, (long long)j);
        P.v[j] = V[j]; P.dv[j] = dV[j];
    }
    for (int64_t t = 0; t < 2 * Q * J; ++t)
        SSQ_REQUIRE(proj[t] - proj[t] == 0.0, "%s: proj[%lld][%lld] is not finite", name, (long long)(t / (2 * J)),
                    (long long)(t / 2 % J));
    if (check_gamma(name, gamma)) return -1;
    SsqParams sp;
    if (fill_params(sp, grid, params, flipud, gamma, cwt ? 1 : 0, name)) return -1;
    const double* rdev = nullptr;
    if (g_conceft_tables.get(proj, (size_t)(2 * Q * J), &rdev)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return dispatch_bool(cwt, [&](auto c) {
            return dispatch_bool(average != 0, [&](auto a) {
                return launch_conceft<T, decltype(a)::value, decltype(c)::value>(P, rowv, rdev, Cx, sp, batch, J, Q, rows, n,
                                                                                as_stream(stream));
            });
        });
    });
}

extern "C" {

int ssq_conceft(int dtype, const void* const* V, const void* const* dV, const void* Sfs, const double* proj, void* Cx,
                int64_t batch, int64_t J, int64_t Q, int64_t rows, int64_t n, double gamma, int grid, const double* params,
                int flipud, int average, void* stream) {
    return conceft_entry(false, "ssq_conceft", dtype, V, dV, Sfs, proj, Cx, batch, J, Q, rows, n, gamma, grid, params,
                         flipud, average, stream);
}

int ssq_conceft_cwt(int dtype, const void* const* W, const void* const* dW, const void* cst, const double* proj, void* Cx,
                    int64_t batch, int64_t J, int64_t Q, int64_t rows, int64_t n, double gamma, int grid,
                    const double* params, int flipud, int average, void* stream) {
    return conceft_entry(true, "ssq_conceft_cwt", dtype, W, dW, cst, proj, Cx, batch, J, Q, rows, n, gamma, grid, params,
                         flipud, average, stream);
}

}  // extern "C"
