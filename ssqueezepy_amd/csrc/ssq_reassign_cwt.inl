// ssq_reassign_cwt.inl -- ssq_reassign_cwt: the reassigned scalogram (Auger, Flandrin 1995) -- the energy of every point
// of a (batch, rows, n) CWT moves along BOTH axes, to the bin of its instantaneous frequency on the synchrosqueezing grid
// and to its group delay. Kernel, launcher and C-ABI entries; included by ssq_time_reassign.hip after ssq_reassign2d.inl,
// whose peak and finish kernels, shift rule, point test, point load and window write-out it shares. include/ssq_hip.h
// states what is computed; DESIGN.md section 4.5.10 the sizing.
//
// What differs from the STFT form is every index: the destination row is bin_from_w of the point's frequency (a log,
// log-piecewise or linear grid), the column shift is scaled by the row's scale, the displacement bound is per row, a row
// weight multiplies the term, and the rows of the LDS window are BINS: the window of a tile of RCW_TR x RCW_TC sources
// starts RCW_HR rows below the smallest home[i] of the tile's rows -- home[i] being where the caller expects the energy
// of row i to land -- and RCW_HC columns left of the tile. A term inside the window is a 64-bit LDS integer add, one
// outside a no-return 64-bit global integer atomic; integer addition is associative, so `home` (and the window itself)
// decides the speed and nothing else.
namespace ssq {

#include "ssq_point_math.inl"

constexpr int RCW_TR = 8, RCW_TC = 256;         // sources of a tile: rows x columns (a column per work-item)
constexpr int RCW_HR = 4, RCW_HC = 64;          // the window's halo: bins below the smallest home and above it + TR; columns
constexpr int RCW_WR = RCW_TR + 2 * RCW_HR, RCW_WC = RCW_TC + 2 * RCW_HC;       // 16 x 384 cells = 48 KiB: three per CU
constexpr int RCW_CHUNK = 3;                    // lines of the write-out a wavefront holds in registers at a time
static_assert(RCW_TC == R2D_TC && RCW_TR % R2D_RP == 0, "the work-item layout of reassign2d_scatter_kernel");

template <typename T, bool VEC, bool WIN>
__global__ __launch_bounds__(R2D_NT) void reassign_cwt_scatter_kernel(
    const T* __restrict__ W, const T* __restrict__ dW, const T* __restrict__ Wd, const double* __restrict__ cst,
    const double* __restrict__ rsc, const int32_t* __restrict__ dmax, const int32_t* __restrict__ home,
    unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ peak, int64_t units, unsigned rows,
    unsigned n, unsigned rtiles, unsigned ctiles, int H, SsqParams sp) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long* win = reinterpret_cast<unsigned long long*>(lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = tid & (RCW_TC - 1), rp = tid / RCW_TC;
    const int64_t omax = (int64_t)rows - 1;

    // the window is cleared once; every unit's write-out leaves it cleared for the next
    if constexpr (WIN) {
        for (int t = tid; t < RCW_WR * RCW_WC; t += R2D_NT) win[t] = 0ull;
        __syncthreads();
    }

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const unsigned ct = (unsigned)(unit % ctiles);
        const int64_t ur = unit / ctiles;
        const unsigned rt = (unsigned)(ur % rtiles), b = (unsigned)(ur / rtiles);
        const unsigned long long pk = peak[b];
        if (!pk) continue;                                      // (workgroup-uniform) no kept point, or every term 0
        const int sh = reassign2d_shift(pk, H);
        const int64_t r0 = (int64_t)rt * RCW_TR;
        const int64_t c0 = (int64_t)ct * RCW_TC, wc0 = c0 - RCW_HC;
        const size_t boff = (size_t)b * rows * (size_t)n;       // (the host guarantees batch rows n < 2^32)
        // the window's first bin: below the smallest home of the tile's rows (any int32 will do: 64-bit from here on)
        int64_t wr0 = 0;
        if constexpr (WIN) {
            int32_t hmin = home[r0];
            for (int j = 1; j < RCW_TR && r0 + j < (int64_t)rows; ++j) hmin = home[r0 + j] < hmin ? home[r0 + j] : hmin;
            wr0 = (int64_t)hmin - RCW_HR;
        }

        const int64_t c = c0 + col;
        if (c < (int64_t)n && r0 + rp < (int64_t)rows) {
            // a row's three points are requested while the row before it is being used
            double ngr = 0., ngi = 0., ndr = 0., ndi = 0., ntr = 0., nti = 0.;
            auto load = [&](int64_t i) {
                const size_t o = boff + (size_t)i * n + (size_t)c;
                reassign2d_load<T, VEC>(W, o, ngr, ngi);
                if (dW) reassign2d_load<T, VEC>(dW, o, ndr, ndi);
                if (Wd) reassign2d_load<T, VEC>(Wd, o, ntr, nti);
            };
            load(r0 + rp);
#pragma unroll
            for (int j = 0; j < RCW_TR / R2D_RP; ++j) {
                const int rr = rp + j * R2D_RP;
                const int64_t i = r0 + rr;
                if (i >= (int64_t)rows) break;
                const double gr = ngr, gi = ngi, dr = ndr, di = ndi, tr = ntr, ti = nti;
                if (rr + R2D_RP < RCW_TR && i + R2D_RP < (int64_t)rows) load(i + R2D_RP);
                double e;
                if (!reassign2d_kept<T>(gr, gi, sp.gamma, e)) continue;
                int64_t k2 = i;
                int d = 0;
                if (dW) {
                    const double w = fabs(phase_ratio(dr, di, gr, gi));             // |Im(dW / W)| / 2 pi
                    k2 = bin_from_w(w, sp, omax);                                   // 0 .. rows - 1, whatever w is
                    if (sp.flipud) k2 = omax - k2;
                }
                if (Wd) {
                    const double s = (ti * gr - tr * gi) / e;                       // Im(Wd / W) = Re(T / W) / r
                    const double dd = rint(s * rsc[i]);
                    if (!(fabs(dd) <= (double)dmax[i])) continue;                   // (NaN included)
                    d = (int)dd;
                }
                const int64_t c2 = c + d;
                if (c2 < 0 || c2 >= (int64_t)n) continue;
                const unsigned long long q = (unsigned long long)ldexp(e * cst[i], sh);
                if (!q) continue;
                const int64_t wr = k2 - wr0;
                const int64_t wc = c2 - wc0;
                if (WIN && wr >= 0 && wr < RCW_WR && wc >= 0 && wc < RCW_WC)
                    __scoped_atomic_fetch_add(win + (int)wr * RCW_WC + (int)wc, q, __ATOMIC_RELAXED, __MEMORY_SCOPE_WRKGRP);
                else
                    __scoped_atomic_fetch_add(acc + boff + (size_t)k2 * n + (size_t)c2, q, __ATOMIC_RELAXED,
                                              __MEMORY_SCOPE_DEVICE);
            }
        }

        if constexpr (WIN) {
            __syncthreads();
            reassign2d_flush_window<RCW_WR, RCW_WC, RCW_CHUNK>(win, acc, boff, wr0, wc0, rows, n, wave, lane);
            __syncthreads();                                    // the next unit adds into the cleared window
        }
    }
}

template <typename T>
static int launch_reassign_cwt(const void* W, const void* dW, const void* Wd, const double* cst, const double* rsc,
                               const int32_t* dmax, const int32_t* home, void* Rx, void* acc, void* peak, int64_t batch,
                               int64_t rows, int64_t n, int H, const SsqParams& sp, bool window, hipStream_t stream) {
    const int64_t plane = rows * n;
    auto* accp = static_cast<unsigned long long*>(acc);
    auto* peakp = static_cast<unsigned long long*>(peak);
    SSQ_CHECK_HIP(hipMemsetAsync(peak, 0, (size_t)batch * 8, stream));
    SSQ_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)batch * (size_t)plane * 8, stream));
    // one load per point needs every plane on a 16-byte boundary (a caller's offset pointer need not be)
    const bool vec = (uintptr_t)W % 16 == 0 && (uintptr_t)dW % 16 == 0 && (uintptr_t)Wd % 16 == 0;
    const unsigned by = (unsigned)(batch < 65535 ? batch : 65535);

    int64_t gx = (plane + 256 * 16 - 1) / (256 * 16);           // 16 points per work-item or more
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    int rc = launch_lds(vec ? reassign2d_peak_kernel<T, true, true> : reassign2d_peak_kernel<T, false, true>,
                        dim3((unsigned)gx, by), dim3(256), 16, stream, (const T*)W, peakp, (unsigned)batch, (unsigned)plane,
                        sp.gamma, cst, (unsigned)n);
    if (rc) return rc;

    const int64_t rtiles = (rows + RCW_TR - 1) / RCW_TR, ctiles = (n + RCW_TC - 1) / RCW_TC, units = batch * rtiles * ctiles;
    // with the window a workgroup clears 48 KiB of LDS once and then walks its units: a few per workgroup
    const int64_t gcap = window ? R2D_MAX_GRID : TSSQ_MAX_GRID;
    const dim3 grid((unsigned)(units < gcap ? units : gcap));
    auto scatter = [&](auto kern, size_t lds) {
        return launch_lds(kern, grid, dim3(R2D_NT), lds, stream, (const T*)W, (const T*)dW, (const T*)Wd, cst, rsc, dmax,
                          home, accp, (const unsigned long long*)peakp, units, (unsigned)rows, (unsigned)n,
                          (unsigned)rtiles, (unsigned)ctiles, H, sp);
    };
    const size_t wbytes = (size_t)RCW_WR * RCW_WC * 8;
    if (window) rc = vec ? scatter(reassign_cwt_scatter_kernel<T, true, true>, wbytes) : scatter(reassign_cwt_scatter_kernel<T, false, true>, wbytes);
    else rc = vec ? scatter(reassign_cwt_scatter_kernel<T, true, false>, 0) : scatter(reassign_cwt_scatter_kernel<T, false, false>, 0);
    if (rc) return rc;

    hipLaunchKernelGGL(reassign2d_finish_kernel<T>, dim3((unsigned)gx, by), dim3(256), 0, stream,
                       (const unsigned long long*)accp, (const unsigned long long*)peakp, (T*)Rx, (unsigned)batch,
                       (unsigned)plane, H);
    SSQ_LAUNCH_CHECK();
    return 0;
}

static DeviceTableCache g_reassign_cwt_tables;      // the rows' dmax

}  // namespace ssq

extern "C" {

int ssq_reassign_cwt_tile(int which) {
    switch (which) {
        case 0: return ssq::RCW_TR;
        case 1: return ssq::RCW_TC;
        case 2: return ssq::RCW_HR;
        case 3: return ssq::RCW_HC;
        case 4: return (int)ssq::R2D_MAX_GRID;
        case 5: return ssq::RCW_WR;
        case 6: return ssq::RCW_WC;
        default: return 0;
    }
}

int ssq_reassign_cwt(int dtype, const void* W, const void* dW, const void* Wd, const double* cst, const double* rsc,
                     const int32_t* dmax, const int32_t* home, void* Rx, void* acc, void* peak, int64_t batch,
                     int64_t rows, int64_t n, double gamma, int grid, const double* params, int flipud, int flags,
                     void* stream) {
    using namespace ssq;
    if (check_dtype(dtype)) return -1;
    const bool freq = (flags & SSQ_REASSIGN_CWT_FREQ) != 0, time = (flags & SSQ_REASSIGN_CWT_TIME) != 0;
    const bool window = !(flags & SSQ_REASSIGN_CWT_NO_WINDOW);
    SSQ_REQUIRE((flags & ~(SSQ_REASSIGN_CWT_FREQ | SSQ_REASSIGN_CWT_TIME | SSQ_REASSIGN_CWT_NO_WINDOW)) == 0,
                "ssq_reassign_cwt: unknown flags %#x", flags);
    SSQ_REQUIRE(W && cst && Rx && acc && peak && (dW || !freq) && ((Wd && rsc && dmax) || !time) && (home || !window) &&
                (params || !freq), "ssq_reassign_cwt: null pointer");
    SSQ_REQUIRE(batch >= 1 && rows >= 2 && n >= 1, "ssq_reassign_cwt: bad shape (%lld, %lld, %lld): batch, n >= 1, rows >= 2",
                (long long)batch, (long long)rows, (long long)n);
    if (check_point_count("ssq_reassign_cwt", batch, rows, n)) return -1;
    if (check_gamma("ssq_reassign_cwt", gamma)) return -1;
    SsqParams sp;
    if (freq) {
        if (fill_params(sp, grid, params, flipud, gamma, 1, "ssq_reassign_cwt")) return -1;
    } else {                                                    // (no bin is taken: the grid is not looked at)
        static const double none[5] = {0., 1., 1., 1., 0.};
        if (fill_params(sp, SSQ_GRID_LIN, none, 0, gamma, 1, "ssq_reassign_cwt")) return -1;
    }
    // C, the most terms a cell can receive: a bin takes the points of every row (the frequency axis on) or of its own row
    // only, from the columns within the row's dmax (at most rows * n, so the point count above already keeps it below
    // 2^32; the limit that the headroom rule itself needs is stated all the same)
    int64_t C = freq ? 0 : 1;
    for (int64_t i = 0; i < rows; ++i) {
        const int64_t dm = time ? (int64_t)dmax[i] : 0;
        SSQ_REQUIRE(dm >= 0 && dm <= TSSQ_MAX_DMAX, "ssq_reassign_cwt: dmax[%lld] = %lld, 0 .. %lld", (long long)i,
                    (long long)dm, (long long)TSSQ_MAX_DMAX);
        const int64_t reach = 2 * dm + 1 < n ? 2 * dm + 1 : n;
        C = freq ? C + reach : (reach > C ? reach : C);
    }
    SSQ_REQUIRE(C < ((int64_t)1 << 40), "ssq_reassign_cwt: %lld terms can meet in a cell, fewer than 2^40", (long long)C);
    int H = 0;
    for (int64_t v = C; v; v >>= 1) ++H;
    const int32_t* dmax_dev = nullptr;
    if (time && g_reassign_cwt_tables.get(dmax, (size_t)rows, &dmax_dev)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_reassign_cwt<T>(W, freq ? dW : nullptr, time ? Wd : nullptr, cst, rsc, dmax_dev, home, Rx, acc, peak,
                                      batch, rows, n, H, sp, window, as_stream(stream));
    });
}

}  // extern "C"
