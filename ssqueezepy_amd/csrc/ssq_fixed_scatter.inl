// ssq_fixed_scatter.inl -- the fixed-point scatter that ssq_reassign2d, ssq_reassign_cwt and ssq_time_reassign_cwt are
// built on: kernels, launcher and the host's headroom helper; included by ssq_time_reassign.hip, whose flags
// (-ffp-contract=off) and point types it shares, ahead of the three entries' files. Those hold a RULE each -- what a
// point becomes -- and nothing of the mechanism. DESIGN.md sections 4.5.9, 4.5.10 and 4.5.12 state the sizing.
//
// The sum of a cell is taken in fixed point: a term is a float64 scaled by 2^sh and truncated to a 64-bit integer, sh
// chosen per signal from the largest kept energy and the most terms a cell can receive so that no cell reaches 2^62.
// Integer addition is associative, so the result does not depend on the order of the additions -- not on the grid, the
// tiling or the schedule -- and atomics may be used freely. Three launches:
//   reassign2d_peak_kernel  the largest (weighted) energy of the kept points of a signal: fetch_max on the double's bits
//                           (energies are non-negative, so the bits order as the values), per workgroup in LDS first,
//                           then one global
//   fixed_scatter_kernel    a workgroup of 512 owns a tile of TR x TC sources (lane = source column: coalesced loads) and
//                           an LDS window of WR x WC destination cells around where the rule expects them to land. A
//                           term that lands in the window is a 64-bit LDS integer add; one that lands outside goes to
//                           the global accumulator with a no-return 64-bit integer atomic. At the tile's end the
//                           window's non-zero words are added to the global accumulator, a wavefront per 64-word line:
//                           runs of neighbouring words (up to 512 bytes per wave instruction), and the window is left
//                           cleared.
//   fixed_finish_kernel     out = (T) ldexp((double) (int64) acc, -sh) per word, full lines
//
// A RULE is a plain struct, passed to the kernel by value:
//   TR, TC, HR, HC, WORDS, CHUNK   the tile's sources, the window's halo in rows and columns, the 64-bit words of a cell
//                           (1: an energy, 2: re and im) and the lines of the write-out a wavefront holds at a time
//   WEIGHTED, cst           whether the peak is taken over e * cst[row]
//   in                      the point's planes (FixedPlanes): the ones that are not null are loaded
//   shift(peak_bits, H)     sh of a signal
//   first_window_row(r0, rows)     the destination row of the window's first line for the tile whose first source row is r0
//   place(p, e, i, c, at, add)     the kept point p of energy e, row i, column c: calls add(k2, c2, {words}) with its
//                           destination cell and term, or returns without if the point is dropped. A word that is 0 is
//                           skipped by `add`. (A continuation, not `bool place(..., k2, c2, q)`: with the flag returned
//                           this compiler lays the unrolled row loop out as nested regions, 17 more exec-mask regions and
//                           80 VGPRs in the float32 STFT instance against 72 so, as before the fold; the window-less
//                           instances would lose a workgroup per CU -- profiles/fixed_scatter_fold.txt.)
#include <cmath>

namespace ssq {

constexpr int FXS_NT = 512, FXS_NW = FXS_NT / 64;       // work-items and wavefronts of a scatter workgroup
constexpr int FXS_TC = 256, FXS_RP = FXS_NT / FXS_TC;   // a work-item per column of a tile; rows per pass
constexpr int64_t FXS_MAX_GRID = 4096;          // workgroups of the windowed scatter: 256 CUs x 3 resident (72 VGPRs) x five rounds or so

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

// A point of up to three planes: the transform, its frequency-axis companion and its time-axis companion. A plane that is
// null is not loaded and its components stay 0.
struct FixedPoint { double gr, gi, dr, di, tr, ti; };
template <typename T>
struct FixedPlanes {
    const T *g, *d, *t;
    template <bool VEC>
    __device__ __forceinline__ void load(size_t o, FixedPoint& p) const {
        reassign2d_load<T, VEC>(g, o, p.gr, p.gi);
        if (d) reassign2d_load<T, VEC>(d, o, p.dr, p.di);
        if (t) reassign2d_load<T, VEC>(t, o, p.tr, p.ti);
    }
    // one load per point needs every plane on a 16-byte boundary (a caller's offset pointer need not be)
    bool aligned() const { return (uintptr_t)g % 16 == 0 && (uintptr_t)d % 16 == 0 && (uintptr_t)t % 16 == 0; }
};

// what `place` is told about the tile: the plane, the tile's column index and the tiles of a row, the work-item's column
// in the tile, sh of the signal
struct FixedAt { unsigned rows, n, ct, ctiles; int col, sh; };

// (WGT: the energy of a point of row i counts as e * cst[i]; n = the row's length)
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

// The end of a tile: the window of WR x WC words whose first word is (wr0, wc0) of the plane is added to `acc` and left
// cleared. A wavefront per line of 64 words, CHUNK lines at a time: the lines are read first, then the non-zero words are
// cleared and added -- runs of neighbouring words, as the terms of a ridge or of noise leave them. Only words of the
// plane hold anything. (All of a wavefront's lines at once cost 120 VGPRs against 72 in the STFT form: two workgroups per
// CU in place of three, and a slower float32 call -- profiles/reassign_stft.txt.) Between two workgroup barriers of the
// caller.
template <int WR, int WC, int CHUNK>
__device__ __forceinline__ void reassign2d_flush_window(unsigned long long* win, unsigned long long* __restrict__ acc,
                                                        size_t boff, int64_t wr0, int64_t wc0, unsigned rows, unsigned n,
                                                        int wave, int lane) {
    constexpr int LINES = WR * (WC / 64) / FXS_NW;
    static_assert(WC % 64 == 0 && (WR * (WC / 64)) % FXS_NW == 0 && LINES % CHUNK == 0, "a line of the window is a wavefront wide");
#pragma unroll 1
    for (int i0 = 0; i0 < LINES; i0 += CHUNK) {
        unsigned long long v[CHUNK];
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) v[i] = win[(wave + FXS_NW * (i0 + i)) * 64 + lane];
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) {
            if (!v[i]) continue;
            const int line = wave + FXS_NW * (i0 + i), wr = line / (WC / 64), ws = line - wr * (WC / 64);
            const int64_t k2 = wr0 + wr;
            const int64_t c2 = wc0 + ws * 64 + lane;
            win[line * 64 + lane] = 0ull;
            if (k2 >= 0 && k2 < (int64_t)rows && c2 >= 0 && c2 < (int64_t)n)
                __scoped_atomic_fetch_add(acc + boff + (size_t)k2 * n + (size_t)c2, v[i], __ATOMIC_RELAXED,
                                          __MEMORY_SCOPE_DEVICE);
        }
    }
}

template <typename T, typename RULE, bool VEC, bool WIN>
__global__ __launch_bounds__(FXS_NT) void fixed_scatter_kernel(
    RULE rule, unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ peak, int64_t units,
    unsigned rows, unsigned n, unsigned rtiles, unsigned ctiles, int H, double gamma) {
    constexpr int TR = RULE::TR, TC = RULE::TC, WORDS = RULE::WORDS;
    constexpr int WR = TR + 2 * RULE::HR, WC = TC + 2 * RULE::HC;
    static_assert(TC == FXS_TC && TR % FXS_RP == 0 && (WORDS == 1 || WORDS == 2), "a work-item per column of the tile");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long* win = reinterpret_cast<unsigned long long*>(lds_raw);      // WR x WC cells of WORDS words
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = tid & (TC - 1), rp = tid / TC;

    // the window is cleared once; every unit's write-out leaves it cleared for the next
    if constexpr (WIN) {
        for (int t = tid; t < WR * WC * WORDS; t += FXS_NT) win[t] = 0ull;
        __syncthreads();
    }

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const unsigned ct = (unsigned)(unit % ctiles);
        const int64_t ur = unit / ctiles;
        const unsigned rt = (unsigned)(ur % rtiles), b = (unsigned)(ur / rtiles);
        const unsigned long long pk = peak[b];
        if (!pk) continue;                                      // (workgroup-uniform) no kept point, or every term 0
        const FixedAt at{rows, n, ct, ctiles, col, RULE::shift(pk, H)};
        // (rows may be close to 2^31: the row arithmetic is 64-bit)
        const int64_t r0 = (int64_t)rt * TR, wr0 = WIN ? rule.first_window_row(r0, rows) : 0;
        const int64_t c0 = (int64_t)ct * TC, wc0 = c0 - RULE::HC;
        const size_t boff = (size_t)b * rows * (size_t)n;       // (the host guarantees batch rows n WORDS < 2^32)

        const int64_t c = c0 + col;
        if (c < (int64_t)n && r0 + rp < (int64_t)rows) {
            // a row's points are requested while the row before it is being used (a tile of one pass has no row before)
            FixedPoint nx{};
            auto load = [&](int64_t i) { rule.in.template load<VEC>(boff + (size_t)i * n + (size_t)c, nx); };
            load(r0 + rp);
#pragma unroll
            for (int j = 0; j < TR / FXS_RP; ++j) {
                const int rr = rp + j * FXS_RP;
                const int64_t i = r0 + rr;
                if (i >= (int64_t)rows) break;
                const FixedPoint p = nx;
                if (rr + FXS_RP < TR && i + FXS_RP < (int64_t)rows) load(i + FXS_RP);
                double e;
                if (!reassign2d_kept<T>(p.gr, p.gi, gamma, e)) continue;
                rule.place(p, e, i, c, at, [&](int64_t k2, int64_t c2, const unsigned long long (&q)[WORDS]) {
                    const int64_t wr = k2 - wr0;
                    const int64_t wc = c2 - wc0;
                    const bool inside = WIN && wr >= 0 && wr < WR && wc >= 0 && wc < WC;
#pragma unroll
                    for (int w = 0; w < WORDS; ++w) {
                        if (!q[w]) continue;
                        if (inside)
                            __scoped_atomic_fetch_add(win + ((int)wr * WC + (int)wc) * WORDS + w, q[w], __ATOMIC_RELAXED,
                                                      __MEMORY_SCOPE_WRKGRP);
                        else
                            __scoped_atomic_fetch_add(acc + WORDS * (boff + (size_t)k2 * n + (size_t)c2) + w, q[w],
                                                      __ATOMIC_RELAXED, __MEMORY_SCOPE_DEVICE);
                    }
                });
            }
        }

        if constexpr (WIN) {
            __syncthreads();
            // (a cell of two words is two neighbouring words of a plane twice as wide: the (rows, 2 n) view)
            reassign2d_flush_window<WR, WORDS * WC, RULE::CHUNK>(win, acc, WORDS * boff, wr0, WORDS * wc0, rows, WORDS * n,
                                                                 wave, lane);
            __syncthreads();                                    // the next unit adds into the cleared window
        }
    }
}

// `acc` and `out` as real planes of `plane` words per signal. The sums of the energy forms are unsigned and stay below
// 2^62 (the headroom proofs of DESIGN.md 4.5.9 and 4.5.12), so reading them as int64 gives the same double.
template <typename T, typename RULE>
__global__ __launch_bounds__(256) void fixed_finish_kernel(const long long* __restrict__ acc,
                                                            const unsigned long long* __restrict__ peak,
                                                            T* __restrict__ out, unsigned batch, unsigned plane, int H) {
    for (unsigned b = blockIdx.y; b < batch; b += gridDim.y) {
        const int sh = RULE::shift(peak[b], H);
        const size_t off = (size_t)b * plane;
        for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < plane; t += (size_t)gridDim.x * 256)
            out[off + t] = (T)ldexp((double)acc[off + t], -sh);
    }
}

// peak, scatter and finish of one call: `out` and `acc` are (batch, rows, n) cells of RULE::WORDS words
template <typename T, typename RULE>
static int launch_fixed_scatter(const RULE& rule, double gamma, void* out, void* acc, void* peak, int64_t batch,
                                int64_t rows, int64_t n, int H, bool window, hipStream_t stream) {
    constexpr int WORDS = RULE::WORDS, WR = RULE::TR + 2 * RULE::HR, WC = RULE::TC + 2 * RULE::HC;
    const int64_t plane = rows * n;
    auto* accp = static_cast<unsigned long long*>(acc);
    auto* peakp = static_cast<unsigned long long*>(peak);
    SSQ_CHECK_HIP(hipMemsetAsync(peak, 0, (size_t)batch * 8, stream));
    SSQ_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)batch * (size_t)plane * WORDS * 8, stream));
    const bool vec = rule.in.aligned();
    const unsigned by = (unsigned)(batch < 65535 ? batch : 65535);
    auto stream_grid_x = [](int64_t items) {                    // 16 items per work-item or more
        const int64_t gx = (items + 256 * 16 - 1) / (256 * 16);
        return (unsigned)(gx < 1 ? 1 : (gx > 4096 ? 4096 : gx));
    };

    const double* cst = nullptr;
    if constexpr (RULE::WEIGHTED) cst = rule.cst;
    int rc = launch_lds(vec ? reassign2d_peak_kernel<T, true, RULE::WEIGHTED> : reassign2d_peak_kernel<T, false, RULE::WEIGHTED>,
                        dim3(stream_grid_x(plane), by), dim3(256), 16, stream, rule.in.g, peakp, (unsigned)batch,
                        (unsigned)plane, gamma, cst, RULE::WEIGHTED ? (unsigned)n : 0u);
    if (rc) return rc;

    const int64_t rtiles = (rows + RULE::TR - 1) / RULE::TR, ctiles = (n + RULE::TC - 1) / RULE::TC, units = batch * rtiles * ctiles;
    // with the window a workgroup clears its 36 or 48 KiB of LDS once and then walks its units: a few per workgroup
    const int64_t gcap = window ? FXS_MAX_GRID : TSSQ_MAX_GRID;
    const dim3 grid((unsigned)(units < gcap ? units : gcap));
    auto scatter = [&](auto kern) {
        return launch_lds(kern, grid, dim3(FXS_NT), window ? (size_t)WR * WC * WORDS * 8 : 0, stream, rule, accp,
                          (const unsigned long long*)peakp, units, (unsigned)rows, (unsigned)n, (unsigned)rtiles,
                          (unsigned)ctiles, H, gamma);
    };
    if (window) rc = vec ? scatter(fixed_scatter_kernel<T, RULE, true, true>) : scatter(fixed_scatter_kernel<T, RULE, false, true>);
    else rc = vec ? scatter(fixed_scatter_kernel<T, RULE, true, false>) : scatter(fixed_scatter_kernel<T, RULE, false, false>);
    if (rc) return rc;

    hipLaunchKernelGGL((fixed_finish_kernel<T, RULE>), dim3(stream_grid_x(WORDS * plane), by), dim3(256), 0, stream,
                       (const long long*)acc, (const unsigned long long*)peakp, (T*)out, (unsigned)batch,
                       (unsigned)(WORDS * plane), H);
    SSQ_LAUNCH_CHECK();
    return 0;
}

// C, the most terms a cell can receive, and H = bit_length(C): a cell takes the points of every row (`sum`) or of its own
// row only, from the columns within the row's dmax -- `dmax` (rows,), or `dmax_all` for every row where it is null. Every
// bound is checked under the entry's `name`.
static int fixed_headroom(const char* name, const int32_t* dmax, int64_t dmax_all, int64_t rows, int64_t n, bool sum,
                          int64_t& C, int& H) {
    const int64_t count = dmax ? rows : 1, each = dmax ? 1 : rows;     // (one bound for every row is looked at once)
    C = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t dm = dmax ? (int64_t)dmax[i] : dmax_all;
        SSQ_REQUIRE(dm >= 0 && dm <= TSSQ_MAX_DMAX, "%s: dmax[%lld] = %lld, 0 .. %lld", name, (long long)i, (long long)dm,
                    (long long)TSSQ_MAX_DMAX);
        const int64_t reach = 2 * dm + 1 < n ? 2 * dm + 1 : n;
        C = sum ? C + each * reach : (reach > C ? reach : C);
    }
    H = 0;
    for (int64_t v = C; v; v >>= 1) ++H;
    return 0;
}

}  // namespace ssq
