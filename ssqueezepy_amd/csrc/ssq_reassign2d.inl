// ssq_reassign2d.inl -- ssq_reassign2d: the reassigned spectrogram (Kodera, Gendrin, de Villedary 1978; Auger, Flandrin
// 1995) -- the energy of every point of a (batch, rows, n) plane moves along BOTH axes, to its instantaneous frequency
// and its group delay. Kernels, launcher and C-ABI entries; included by ssq_time_reassign.hip, whose flags
// (-ffp-contract=off) and point types it shares. include/ssq_hip.h states what is computed; DESIGN.md section 4.5.9 the
// sizing.
//
// The sum of a cell is taken in fixed point: a term is the energy scaled by 2^sh and truncated to a uint64, sh chosen
// per signal from the largest energy and the most terms a cell can receive so that no cell reaches 2^62. Integer
// addition is associative, so the result does not depend on the order of the additions -- not on the grid, the tiling
// or the schedule -- and atomics may be used freely. Three launches:
//   reassign2d_peak     the largest energy of the kept points of a signal: fetch_max on the double's bits (energies are
//                       non-negative, so the bits order as the values), per workgroup in LDS first, then one global
//   reassign2d_scatter  a workgroup of 512 owns a tile of R2D_TR x R2D_TC sources (lane = source column: coalesced
//                       loads) and an LDS window of destination cells R2D_HR rows and R2D_HC columns wider on every
//                       side. A term that lands in the window is a 64-bit LDS integer add; one that lands outside goes
//                       to the global accumulator with a no-return 64-bit integer atomic. At the tile's end the window's
//                       non-zero cells are added to the global accumulator, a wavefront per 64-cell line: runs of
//                       neighbouring cells (up to 512 bytes per wave instruction), and the window is left cleared.
//   reassign2d_finish   Rx = (T) ldexp((double) acc, -sh), full lines
#include <cmath>

namespace ssq {

constexpr int R2D_TR = 8, R2D_TC = 256;         // sources of a tile: rows x columns (a column per work-item)
constexpr int R2D_HR = 2, R2D_HC = 64;          // the window's halo: rows above and below, columns left and right
constexpr int R2D_NT = 512, R2D_NW = R2D_NT / 64, R2D_RP = R2D_NT / R2D_TC;     // work-items, wavefronts, rows per pass
constexpr int R2D_WR = R2D_TR + 2 * R2D_HR, R2D_WC = R2D_TC + 2 * R2D_HC;     // 12 x 384 cells = 36 KiB
constexpr double R2D_TWO_PI = 6.283185307179586;
constexpr int64_t R2D_MAX_GRID = 4096;         // workgroups of the windowed scatter: 256 CUs x 3 resident (72 VGPRs) x five rounds or so
constexpr int R2D_LINES = R2D_WR * (R2D_WC / 64) / R2D_NW;      // lines of 64 cells per wavefront at the write-out
constexpr int R2D_CHUNK = 3;                    // ... of which a wavefront holds this many in registers at a time
static_assert(R2D_WC % 64 == 0 && R2D_TC == 256 && R2D_TR % R2D_RP == 0 && (R2D_WR * (R2D_WC / 64)) % R2D_NW == 0 && R2D_LINES % R2D_CHUNK == 0, "a line of the window is a wavefront wide; a work-item per column");

// sh of a signal from its peak word (the bits of the largest kept energy) and H = bit_length(terms a cell can receive)
__device__ __forceinline__ int reassign2d_shift(unsigned long long peak_bits, int H) {
    int ex = 0;
    (void)frexp(__builtin_bit_cast(double, peak_bits), &ex);
    return 62 - H - ex;
}

// the energy of a point and whether it is kept
template <typename T>
__device__ __forceinline__ bool reassign2d_kept(double gr, double gi, double gamma, double& e) {
    e = gr * gr + gi * gi;
    return !(phase2_abs(gr, gi, T(0)) < gamma) && e <= DBL_MAX;          // (false for a NaN or infinite e)
}

template <typename T, bool VEC>
__device__ __forceinline__ void reassign2d_load(const T* __restrict__ P, size_t o, double& re, double& im) {
    using load_t = std::conditional_t<sizeof(T) == 4, phase2_f2v, phase2_d2v>;      // one complex point
    if constexpr (VEC) {
        const load_t g = reinterpret_cast<const load_t*>(P)[o];
        re = (double)g.x; im = (double)g.y;
    } else {
        re = (double)P[2 * o]; im = (double)P[2 * o + 1];
    }
}

// (WGT: the energy of a point of row i counts as e * cst[i], the term ssq_reassign_cwt adds; n = the row's length)
template <typename T, bool VEC, bool WGT>
__global__ __launch_bounds__(256) void reassign2d_peak_kernel(const T* __restrict__ Sx, unsigned long long* __restrict__ peak,
                                                               unsigned batch, unsigned plane, double gamma,
                                                               const double* __restrict__ cst, unsigned n) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long* top = reinterpret_cast<unsigned long long*>(lds_raw);
    for (unsigned b = blockIdx.y; b < batch; b += gridDim.y) {
        if (threadIdx.x == 0) top[0] = 0ull;
        __syncthreads();
        unsigned long long best = 0ull;
        const size_t off = (size_t)b * plane;
        for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < plane; t += (size_t)gridDim.x * 256) {
            double gr, gi, e;
            reassign2d_load<T, VEC>(Sx, off + t, gr, gi);
            if (reassign2d_kept<T>(gr, gi, gamma, e)) {
                if constexpr (WGT) e = e * cst[t / n];
                const unsigned long long bits = __builtin_bit_cast(unsigned long long, e);
                best = bits > best ? bits : best;
            }
        }
        if (best) __scoped_atomic_fetch_max(top, best, __ATOMIC_RELAXED, __MEMORY_SCOPE_WRKGRP);
        __syncthreads();
        if (threadIdx.x == 0 && top[0])
            __scoped_atomic_fetch_max(peak + b, top[0], __ATOMIC_RELAXED, __MEMORY_SCOPE_DEVICE);
        __syncthreads();                                        // (thread 0 has read top[0] before the next signal clears it)
    }
}

// The end of a tile, shared with reassign_cwt_scatter_kernel (ssq_reassign_cwt.inl): the window of WR x WC cells whose
// first cell is (wr0, wc0) of the plane is added to `acc` and left cleared. A wavefront per line of 64 cells, CHUNK lines
// at a time: the lines are read first, then the non-zero cells are cleared and added -- runs of neighbouring cells, as
// the terms of a ridge or of noise leave them. Only cells of the plane hold anything. (All of a wavefront's lines at once
// cost 120 VGPRs against 72 in the STFT form: two workgroups per CU in place of three, and a slower float32 call --
// profiles/reassign_stft.txt.) Between two workgroup barriers of the caller.
template <int WR, int WC, int CHUNK>
__device__ __forceinline__ void reassign2d_flush_window(unsigned long long* win, unsigned long long* __restrict__ acc,
                                                        size_t boff, int64_t wr0, int64_t wc0, unsigned rows, unsigned n,
                                                        int wave, int lane) {
    constexpr int LINES = WR * (WC / 64) / R2D_NW;
    static_assert(WC % 64 == 0 && (WR * (WC / 64)) % R2D_NW == 0 && LINES % CHUNK == 0, "a line of the window is a wavefront wide");
#pragma unroll 1
    for (int i0 = 0; i0 < LINES; i0 += CHUNK) {
        unsigned long long v[CHUNK];
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) v[i] = win[(wave + R2D_NW * (i0 + i)) * 64 + lane];
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) {
            if (!v[i]) continue;
            const int line = wave + R2D_NW * (i0 + i), wr = line / (WC / 64), ws = line - wr * (WC / 64);
            const int64_t k2 = wr0 + wr;
            const int64_t c2 = wc0 + ws * 64 + lane;
            win[line * 64 + lane] = 0ull;
            if (k2 >= 0 && k2 < (int64_t)rows && c2 >= 0 && c2 < (int64_t)n)
                __scoped_atomic_fetch_add(acc + boff + (size_t)k2 * n + (size_t)c2, v[i], __ATOMIC_RELAXED,
                                          __MEMORY_SCOPE_DEVICE);
        }
    }
}

template <typename T, bool VEC, bool WIN>
__global__ __launch_bounds__(R2D_NT) void reassign2d_scatter_kernel(
    const T* __restrict__ Sx, const T* __restrict__ dSx, const T* __restrict__ Vtg, unsigned long long* __restrict__ acc,
    const unsigned long long* __restrict__ peak, int64_t units, unsigned rows, unsigned n, unsigned rtiles, unsigned ctiles,
    int H, double df, double cps, int64_t kmax, int dmax, double gamma) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long* win = reinterpret_cast<unsigned long long*>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = tid & (R2D_TC - 1), rp = tid / R2D_TC;

    // the window is cleared once; every unit's write-out leaves it cleared for the next
    if constexpr (WIN) {
        for (int t = tid; t < R2D_WR * R2D_WC; t += R2D_NT) win[t] = 0ull;
        __syncthreads();
    }

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const unsigned ct = (unsigned)(unit % ctiles);
        const int64_t ur = unit / ctiles;
        const unsigned rt = (unsigned)(ur % rtiles), b = (unsigned)(ur / rtiles);
        const unsigned long long pk = peak[b];
        if (!pk) continue;                                      // (workgroup-uniform) no kept point, or every energy 0
        const int sh = reassign2d_shift(pk, H);
        // (rows may be close to 2^31: the row arithmetic is 64-bit)
        const int64_t r0 = (int64_t)rt * R2D_TR, wr0 = r0 - R2D_HR;
        const int64_t c0 = (int64_t)ct * R2D_TC, wc0 = c0 - R2D_HC;
        const size_t boff = (size_t)b * rows * (size_t)n;       // (the host guarantees batch rows n < 2^32)

        const int64_t c = c0 + col;
        if (c < (int64_t)n && r0 + rp < (int64_t)rows) {
            // a row's three points are requested while the row before it is being used
            double ngr = 0., ngi = 0., ndr = 0., ndi = 0., ntr = 0., nti = 0.;
            auto load = [&](int64_t k) {
                const size_t o = boff + (size_t)k * n + (size_t)c;
                reassign2d_load<T, VEC>(Sx, o, ngr, ngi);
                if (dSx) reassign2d_load<T, VEC>(dSx, o, ndr, ndi);
                if (Vtg) reassign2d_load<T, VEC>(Vtg, o, ntr, nti);
            };
            load(r0 + rp);
#pragma unroll
            for (int j = 0; j < R2D_TR / R2D_RP; ++j) {
                const int rr = rp + j * R2D_RP;
                const int64_t k = r0 + rr;
                if (k >= (int64_t)rows) break;
                const double gr = ngr, gi = ngi, dr = ndr, di = ndi, tr = ntr, ti = nti;
                if (rr + R2D_RP < R2D_TR && k + R2D_RP < (int64_t)rows) load(k + R2D_RP);
                double e;
                if (!reassign2d_kept<T>(gr, gi, gamma, e)) continue;
                int64_t m = 0;
                int d = 0;
                if (dSx) {
                    const double im = (di * gr - dr * gi) / e;                      // Im(dSx / Sx)
                    const double mf = rint(((-im) / R2D_TWO_PI) / df);
                    if (!(fabs(mf) <= (double)kmax)) continue;                      // (NaN included)
                    m = (int64_t)mf;
                }
                if (Vtg) {
                    const double s = (tr * gr + ti * gi) / e;                       // Re(Vtg / Sx)
                    const double dd = rint(s * cps);
                    if (!(fabs(dd) <= (double)dmax)) continue;
                    d = (int)dd;
                }
                int64_t k2 = k + m;
                k2 = k2 < 0 ? -k2 : k2;
                const int64_t c2 = c + d;
                if (k2 > (int64_t)rows - 1 || c2 < 0 || c2 >= (int64_t)n) continue;
                const unsigned long long q = (unsigned long long)ldexp(e, sh);
                if (!q) continue;
                const int64_t wr = k2 - wr0;
                const int64_t wc = c2 - wc0;
                if (WIN && wr >= 0 && wr < R2D_WR && wc >= 0 && wc < R2D_WC)
                    __scoped_atomic_fetch_add(win + (int)wr * R2D_WC + (int)wc, q, __ATOMIC_RELAXED, __MEMORY_SCOPE_WRKGRP);
                else
                    __scoped_atomic_fetch_add(acc + boff + (size_t)k2 * n + (size_t)c2, q, __ATOMIC_RELAXED,
                                              __MEMORY_SCOPE_DEVICE);
            }
        }

        if constexpr (WIN) {
            __syncthreads();
            reassign2d_flush_window<R2D_WR, R2D_WC, R2D_CHUNK>(win, acc, boff, wr0, wc0, rows, n, wave, lane);
            __syncthreads();                                    // the next unit adds into the cleared window
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void reassign2d_finish_kernel(const unsigned long long* __restrict__ acc,
                                                                 const unsigned long long* __restrict__ peak,
                                                                 T* __restrict__ Rx, unsigned batch, unsigned plane, int H) {
    for (unsigned b = blockIdx.y; b < batch; b += gridDim.y) {
        const int sh = reassign2d_shift(peak[b], H);
        const size_t off = (size_t)b * plane;
        for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < plane; t += (size_t)gridDim.x * 256)
            Rx[off + t] = (T)ldexp((double)acc[off + t], -sh);
    }
}

template <typename T>
static int launch_reassign2d(const void* Sx, const void* dSx, const void* Vtg, void* Rx, void* acc, void* peak,
                             int64_t batch, int64_t rows, int64_t n, int H, double df, double cps, int64_t kmax,
                             int64_t dmax, double gamma, bool window, hipStream_t stream) {
    const int64_t plane = rows * n;
    auto* accp = static_cast<unsigned long long*>(acc);
    auto* peakp = static_cast<unsigned long long*>(peak);
    SSQ_CHECK_HIP(hipMemsetAsync(peak, 0, (size_t)batch * 8, stream));
    SSQ_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)batch * (size_t)plane * 8, stream));
    // one load per point needs every plane on a 16-byte boundary (a caller's offset pointer need not be)
    const bool vec = (uintptr_t)Sx % 16 == 0 && (uintptr_t)dSx % 16 == 0 && (uintptr_t)Vtg % 16 == 0;
    const unsigned by = (unsigned)(batch < 65535 ? batch : 65535);

    int64_t gx = (plane + 256 * 16 - 1) / (256 * 16);           // 16 points per work-item or more
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    int rc = launch_lds(vec ? reassign2d_peak_kernel<T, true, false> : reassign2d_peak_kernel<T, false, false>,
                        dim3((unsigned)gx, by), dim3(256), 16, stream, (const T*)Sx, peakp, (unsigned)batch, (unsigned)plane,
                        gamma, (const double*)nullptr, 0u);
    if (rc) return rc;

    const int64_t rtiles = (rows + R2D_TR - 1) / R2D_TR, ctiles = (n + R2D_TC - 1) / R2D_TC, units = batch * rtiles * ctiles;
    // with the window a workgroup clears 36 KiB of LDS once and then walks its units: a few per workgroup
    const int64_t gcap = window ? R2D_MAX_GRID : TSSQ_MAX_GRID;
    const dim3 grid((unsigned)(units < gcap ? units : gcap));
    // |k + m| <= rows - 1 needs |m| <= 2 (rows - 1): a larger kmax changes nothing and m stays below 2^33 (the kernel's
    // row arithmetic is 64-bit)
    const int64_t km = kmax < 2 * rows ? kmax : 2 * rows;
    auto scatter = [&](auto kern, size_t lds) {
        return launch_lds(kern, grid, dim3(R2D_NT), lds, stream, (const T*)Sx, (const T*)dSx, (const T*)Vtg, accp,
                          (const unsigned long long*)peakp, units, (unsigned)rows, (unsigned)n, (unsigned)rtiles,
                          (unsigned)ctiles, H, df, cps, km, (int)dmax, gamma);
    };
    const size_t wbytes = (size_t)R2D_WR * R2D_WC * 8;
    if (window) rc = vec ? scatter(reassign2d_scatter_kernel<T, true, true>, wbytes) : scatter(reassign2d_scatter_kernel<T, false, true>, wbytes);
    else rc = vec ? scatter(reassign2d_scatter_kernel<T, true, false>, 0) : scatter(reassign2d_scatter_kernel<T, false, false>, 0);
    if (rc) return rc;

    hipLaunchKernelGGL(reassign2d_finish_kernel<T>, dim3((unsigned)gx, by), dim3(256), 0, stream,
                       (const unsigned long long*)accp, (const unsigned long long*)peakp, (T*)Rx, (unsigned)batch,
                       (unsigned)plane, H);
    SSQ_LAUNCH_CHECK();
    return 0;
}

}  // namespace ssq

extern "C" {

int ssq_reassign2d_tile(int which) {
    switch (which) {
        case 0: return ssq::R2D_TR;
        case 1: return ssq::R2D_TC;
        case 2: return ssq::R2D_HR;
        case 3: return ssq::R2D_HC;
        case 4: return (int)ssq::R2D_MAX_GRID;
        default: return 0;
    }
}

int ssq_reassign2d(int dtype, const void* Sx, const void* dSx, const void* Vtg, void* Rx, void* acc, void* peak,
                   int64_t batch, int64_t rows, int64_t n, int64_t n_fft, int64_t hop_len, double fs,
                   double cols_per_second, int64_t kmax, int64_t dmax, double gamma, int flags, void* stream) {
    using namespace ssq;
    if (check_dtype(dtype)) return -1;
    const bool freq = (flags & SSQ_REASSIGN2D_FREQ) != 0;
    SSQ_REQUIRE((flags & ~(SSQ_REASSIGN2D_FREQ | SSQ_REASSIGN2D_NO_WINDOW)) == 0, "ssq_reassign2d: unknown flags %#x", flags);
    SSQ_REQUIRE(Sx && Rx && acc && peak && (dSx || !freq) && (Vtg || dmax == 0), "ssq_reassign2d: null pointer");
    SSQ_REQUIRE(batch >= 1 && rows >= 1 && n >= 1, "ssq_reassign2d: bad shape (%lld, %lld, %lld): batch, rows, n >= 1",
                (long long)batch, (long long)rows, (long long)n);
    if (check_point_count("ssq_reassign2d", batch, rows, n)) return -1;
    SSQ_REQUIRE(n_fft >= 1 && n_fft <= (int64_t)0x7FFFFFFF && hop_len >= 1,
                "ssq_reassign2d: n_fft = %lld, hop_len = %lld: n_fft 1 .. 2^31 - 1, hop_len >= 1", (long long)n_fft,
                (long long)hop_len);
    SSQ_REQUIRE(rows <= n_fft, "ssq_reassign2d: %lld rows of an n_fft of %lld", (long long)rows, (long long)n_fft);
    SSQ_REQUIRE(dmax >= 0 && dmax <= TSSQ_MAX_DMAX, "ssq_reassign2d: dmax = %lld, 0 .. %lld", (long long)dmax,
                (long long)TSSQ_MAX_DMAX);
    SSQ_REQUIRE(kmax >= 0, "ssq_reassign2d: kmax = %lld, >= 0", (long long)kmax);
    SSQ_REQUIRE(fs > 0.0 && fs <= DBL_MAX, "ssq_reassign2d: fs must be positive and finite (got %g)", fs);
    SSQ_REQUIRE(cols_per_second > 0.0 && cols_per_second <= DBL_MAX,
                "ssq_reassign2d: cols_per_second must be positive and finite (got %g)", cols_per_second);
    if (check_gamma("ssq_reassign2d", gamma)) return -1;
    // the terms a cell can receive: every row, from the columns within dmax (at most rows * n, so the point count above
    // already keeps it below 2^32; the limit that the headroom rule itself needs is stated all the same)
    const int64_t reach = 2 * dmax + 1 < n ? 2 * dmax + 1 : n, cell_terms = rows * reach;
    SSQ_REQUIRE(cell_terms < ((int64_t)1 << 40), "ssq_reassign2d: %lld rows x %lld columns can meet in a cell, fewer than 2^40",
                (long long)rows, (long long)reach);
    int H = 0;
    for (int64_t v = cell_terms; v; v >>= 1) ++H;
    const double df = fs / (double)n_fft;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_reassign2d<T>(Sx, freq ? dSx : nullptr, dmax ? Vtg : nullptr, Rx, acc, peak, batch, rows, n, H, df,
                                    cols_per_second, kmax, dmax, gamma, !(flags & SSQ_REASSIGN2D_NO_WINDOW),
                                    as_stream(stream));
    });
}

}  // extern "C"
