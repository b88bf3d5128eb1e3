// ssq_time_reassign_cwt.inl -- ssq_time_reassign_cwt: the time-reassigned synchrosqueezed CWT -- every coefficient of a
// (batch, rows, n) CWT moves along its row to its group delay, rotated to the signal's origin first so that the terms
// that meet in a cell add coherently. Kernels, launcher and C-ABI entries; included by ssq_time_reassign.hip after
// ssq_reassign_cwt.inl, whose peak kernel, point test, point load and window write-out (ssq_reassign2d.inl) it shares.
// include/ssq_hip.h states what is computed; DESIGN.md section 4.5.12 the sizing.
//
// The STFT form (time_reassign_kernel, above) owns a strip of destination cells and re-reads 960 + 2 dmax sources per
// strip with one scalar dmax; a CWT row's bound grows with its scale to thousands of columns, so the sum here is
// order-free instead: ssq_reassign_cwt's fixed-point accumulator carried over to signed complex terms. `acc` holds re and
// im interleaved, so it is a real plane of 2 n columns, and two's-complement addition is unsigned addition: the window
// write-out of the energy forms serves unchanged on that view.
//
// The rotation e^{-2 pi i phi_i c} comes from two tables of the caller's, rot_lo (rows, P) and rot_hi (rows, ceil(n / P)):
// a tile starts at a multiple of P = its width, so rot_hi is workgroup-uniform per row and rot_lo one load per lane.
namespace ssq {

constexpr int TCW_P = SSQ_TSSQ_CWT_ROT_P;       // columns of rot_lo: the period of the two-level rotation table
constexpr int TCW_TR = 2, TCW_TC = 256;         // sources of a tile: rows x columns (a column per work-item, both rows in one pass)
constexpr int TCW_HC = 640;                     // the window's halo in columns, on either side (no row halo: a point stays in its row)
constexpr int TCW_WC = TCW_TC + 2 * TCW_HC;     // 2 x 1536 cells of 16 bytes = 48 KiB: three per CU (the widest of the five
                                                // shapes measured and the fastest: profiles/tssq_cwt.txt)
constexpr int TCW_CHUNK = 3;                    // lines of the write-out a wavefront holds in registers at a time
static_assert(TCW_TC == R2D_TC && TCW_TR == R2D_RP, "a work-item per source of the tile: reassign2d_scatter_kernel's layout, one pass");
static_assert(TCW_TC == TCW_P, "a tile starts at a multiple of P: rot_hi is uniform over a tile's row");

// sh of a signal from its peak word (the bits of the largest kept |W|^2) and H = bit_length(terms a cell can receive):
// a component of a term is below 2^hx (1 + a few ulp), hx = ceil(ex / 2)
__device__ __forceinline__ int time_reassign_cwt_shift(unsigned long long peak_bits, int H) {
    int ex = 0;
    (void)frexp(__builtin_bit_cast(double, peak_bits), &ex);
    return 61 - H - ((ex + 1) >> 1);                            // (an arithmetic shift: the ceiling for either sign)
}

template <typename T, bool VEC, bool WIN>
__global__ __launch_bounds__(R2D_NT) void time_reassign_cwt_scatter_kernel(
    const T* __restrict__ W, const T* __restrict__ Wd, const double* __restrict__ rsc, const int32_t* __restrict__ dmax,
    const double* __restrict__ rot_lo, const double* __restrict__ rot_hi, unsigned long long* __restrict__ acc,
    const unsigned long long* __restrict__ peak, int64_t units, unsigned rows, unsigned n, unsigned rtiles,
    unsigned ctiles, int H, double gamma) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long* win = reinterpret_cast<unsigned long long*>(lds_raw);      // TCW_TR x TCW_WC cells of (re, im)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = tid & (TCW_TC - 1), rp = tid / TCW_TC;

    // the window is cleared once; every unit's write-out leaves it cleared for the next
    if constexpr (WIN) {
        for (int t = tid; t < TCW_TR * TCW_WC * 2; t += R2D_NT) win[t] = 0ull;
        __syncthreads();
    }

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const unsigned ct = (unsigned)(unit % ctiles);
        const int64_t ur = unit / ctiles;
        const unsigned rt = (unsigned)(ur % rtiles), b = (unsigned)(ur / rtiles);
        const unsigned long long pk = peak[b];
        if (!pk) continue;                                      // (workgroup-uniform) no kept point, or every term 0
        const int sh = time_reassign_cwt_shift(pk, H);
        const int64_t r0 = (int64_t)rt * TCW_TR;
        const int64_t c0 = (int64_t)ct * TCW_TC, wc0 = c0 - TCW_HC;
        const size_t boff = (size_t)b * rows * (size_t)n;       // (the host guarantees 2 batch rows n < 2^32)

        // a tile is as many rows as a workgroup takes in one pass: a work-item has one point of row r0 + rp, no row loop
        const int64_t c = c0 + col, i = r0 + rp;
        [&] {
            if (c >= (int64_t)n || i >= (int64_t)rows) return;
            const size_t o = boff + (size_t)i * n + (size_t)c;
            double gr, gi, tr, ti, e;
            reassign2d_load<T, VEC>(W, o, gr, gi);
            reassign2d_load<T, VEC>(Wd, o, tr, ti);
            if (!reassign2d_kept<T>(gr, gi, gamma, e)) return;
            const double s = (ti * gr - tr * gi) / e;                               // Im(Wd / W) = Re(T / W) / r
            const double dd = rint(s * rsc[i]);
            if (!(fabs(dd) <= (double)dmax[i])) return;                             // (NaN included)
            const int64_t c2 = c + (int)dd;
            if (c2 < 0 || c2 >= (int64_t)n) return;
            double ur = 1., ui = 0.;
            if (rot_lo) {
                const size_t l = 2 * ((size_t)i * TCW_P + (size_t)col), h = 2 * ((size_t)i * ctiles + ct);
                const double lr = rot_lo[l], li = rot_lo[l + 1], hr = rot_hi[h], hi = rot_hi[h + 1];
                ur = hr * lr - hi * li; ui = hr * li + hi * lr;
            }
            const double zr = ur * gr - ui * gi, zi = ur * gi + ui * gr;
            // (|z| 2^sh < 2^62: the cast truncates toward zero; two's complement, so the sum may be taken unsigned)
            const unsigned long long qr = (unsigned long long)(long long)ldexp(zr, sh);
            const unsigned long long qi = (unsigned long long)(long long)ldexp(zi, sh);
            const int64_t wc = c2 - wc0;
            if (WIN && wc >= 0 && wc < TCW_WC) {
                unsigned long long* cell = win + (rp * TCW_WC + (int)wc) * 2;
                if (qr) __scoped_atomic_fetch_add(cell, qr, __ATOMIC_RELAXED, __MEMORY_SCOPE_WRKGRP);
                if (qi) __scoped_atomic_fetch_add(cell + 1, qi, __ATOMIC_RELAXED, __MEMORY_SCOPE_WRKGRP);
            } else {
                unsigned long long* cell = acc + 2 * (boff + (size_t)i * n + (size_t)c2);
                if (qr) __scoped_atomic_fetch_add(cell, qr, __ATOMIC_RELAXED, __MEMORY_SCOPE_DEVICE);
                if (qi) __scoped_atomic_fetch_add(cell + 1, qi, __ATOMIC_RELAXED, __MEMORY_SCOPE_DEVICE);
            }
        }();

        if constexpr (WIN) {
            __syncthreads();
            // the (rows, 2 n) view: a cell is two neighbouring reals of a plane twice as wide
            reassign2d_flush_window<TCW_TR, 2 * TCW_WC, TCW_CHUNK>(win, acc, 2 * boff, r0, 2 * wc0, rows, 2u * n, wave, lane);
            __syncthreads();                                    // the next unit adds into the cleared window
        }
    }
}

// Tx = (T) ldexp((double) (int64) acc, -sh), per component: `acc` and `Tx` as real planes of 2 n columns, full lines
template <typename T>
__global__ __launch_bounds__(256) void time_reassign_cwt_finish_kernel(const long long* __restrict__ acc,
                                                                        const unsigned long long* __restrict__ peak,
                                                                        T* __restrict__ Tx, unsigned batch, unsigned plane2,
                                                                        int H) {
    for (unsigned b = blockIdx.y; b < batch; b += gridDim.y) {
        const int sh = time_reassign_cwt_shift(peak[b], H);
        const size_t off = (size_t)b * plane2;
        for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < plane2; t += (size_t)gridDim.x * 256)
            Tx[off + t] = (T)ldexp((double)acc[off + t], -sh);
    }
}

template <typename T>
static int launch_time_reassign_cwt(const void* W, const void* Wd, const double* rsc, const int32_t* dmax,
                                    const void* rot_lo, const void* rot_hi, void* Tx, void* acc, void* peak, int64_t batch,
                                    int64_t rows, int64_t n, int H, double gamma, bool window, hipStream_t stream) {
    const int64_t plane = rows * n;
    auto* accp = static_cast<unsigned long long*>(acc);
    auto* peakp = static_cast<unsigned long long*>(peak);
    SSQ_CHECK_HIP(hipMemsetAsync(peak, 0, (size_t)batch * 8, stream));
    SSQ_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)batch * (size_t)plane * 16, stream));
    // one load per point needs every plane on a 16-byte boundary (a caller's offset pointer need not be)
    const bool vec = (uintptr_t)W % 16 == 0 && (uintptr_t)Wd % 16 == 0;
    const unsigned by = (unsigned)(batch < 65535 ? batch : 65535);

    int64_t gx = (plane + 256 * 16 - 1) / (256 * 16);           // 16 points per work-item or more
    gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
    int rc = launch_lds(vec ? reassign2d_peak_kernel<T, true, false> : reassign2d_peak_kernel<T, false, false>,
                        dim3((unsigned)gx, by), dim3(256), 16, stream, (const T*)W, peakp, (unsigned)batch, (unsigned)plane,
                        gamma, (const double*)nullptr, 0u);
    if (rc) return rc;

    const int64_t rtiles = (rows + TCW_TR - 1) / TCW_TR, ctiles = (n + TCW_TC - 1) / TCW_TC, units = batch * rtiles * ctiles;
    // with the window a workgroup clears 48 KiB of LDS once and then walks its units: a few per workgroup
    const int64_t gcap = window ? R2D_MAX_GRID : TSSQ_MAX_GRID;
    const dim3 grid((unsigned)(units < gcap ? units : gcap));
    auto scatter = [&](auto kern, size_t lds) {
        return launch_lds(kern, grid, dim3(R2D_NT), lds, stream, (const T*)W, (const T*)Wd, rsc, dmax,
                          (const double*)rot_lo, (const double*)rot_hi, accp, (const unsigned long long*)peakp, units,
                          (unsigned)rows, (unsigned)n, (unsigned)rtiles, (unsigned)ctiles, H, gamma);
    };
    const size_t wbytes = (size_t)TCW_TR * TCW_WC * 16;
    if (window) rc = vec ? scatter(time_reassign_cwt_scatter_kernel<T, true, true>, wbytes) : scatter(time_reassign_cwt_scatter_kernel<T, false, true>, wbytes);
    else rc = vec ? scatter(time_reassign_cwt_scatter_kernel<T, true, false>, 0) : scatter(time_reassign_cwt_scatter_kernel<T, false, false>, 0);
    if (rc) return rc;

    int64_t fx = (2 * plane + 256 * 16 - 1) / (256 * 16);
    fx = fx < 1 ? 1 : (fx > 4096 ? 4096 : fx);
    hipLaunchKernelGGL(time_reassign_cwt_finish_kernel<T>, dim3((unsigned)fx, by), dim3(256), 0, stream,
                       (const long long*)acc, (const unsigned long long*)peakp, (T*)Tx, (unsigned)batch,
                       (unsigned)(2 * plane), H);
    SSQ_LAUNCH_CHECK();
    return 0;
}

static DeviceTableCache g_time_reassign_cwt_tables;     // the rows' dmax

}  // namespace ssq

extern "C" {

int ssq_time_reassign_cwt_tile(int which) {
    switch (which) {
        case 0: return ssq::TCW_TR;
        case 1: return ssq::TCW_TC;
        case 2: return ssq::TCW_HC;
        case 3: return ssq::TCW_WC;
        case 4: return (int)ssq::R2D_MAX_GRID;
        case 5: return ssq::TCW_P;
        default: return 0;
    }
}

int ssq_time_reassign_cwt(int dtype, const void* W, const void* Wd, const double* rsc, const int32_t* dmax,
                          const void* rot_lo, const void* rot_hi, void* Tx, void* acc, void* peak, int64_t batch,
                          int64_t rows, int64_t n, double gamma, int flags, void* stream) {
    using namespace ssq;
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE((flags & ~SSQ_TSSQ_CWT_NO_WINDOW) == 0, "ssq_time_reassign_cwt: unknown flags %#x", flags);
    SSQ_REQUIRE(W && Wd && rsc && dmax && Tx && acc && peak, "ssq_time_reassign_cwt: null pointer");
    SSQ_REQUIRE(!rot_lo == !rot_hi, "ssq_time_reassign_cwt: rot_lo and rot_hi go together: both tables or neither");
    SSQ_REQUIRE(batch >= 1 && rows >= 1 && n >= 1,
                "ssq_time_reassign_cwt: bad shape (%lld, %lld, %lld): batch, rows, n >= 1", (long long)batch,
                (long long)rows, (long long)n);
    // (a cell is two words of the (rows, 2 n) view, whose indices the write-out keeps in 32 bits)
    SSQ_REQUIRE(n <= (int64_t)0x7FFFFFFFll && rows <= (int64_t)0x7FFFFFFFll / n && batch <= (int64_t)0x7FFFFFFFll / (rows * n),
                "ssq_time_reassign_cwt: %lld x %lld x %lld points, at most 2^31 - 1", (long long)batch, (long long)rows,
                (long long)n);
    if (check_gamma("ssq_time_reassign_cwt", gamma)) return -1;
    // C, the most terms a cell can receive: the points of its own row from the columns within the row's dmax
    int64_t C = 1;
    for (int64_t i = 0; i < rows; ++i) {
        const int64_t dm = (int64_t)dmax[i];
        SSQ_REQUIRE(dm >= 0 && dm <= TSSQ_MAX_DMAX, "ssq_time_reassign_cwt: dmax[%lld] = %lld, 0 .. %lld", (long long)i,
                    (long long)dm, (long long)TSSQ_MAX_DMAX);
        const int64_t reach = 2 * dm + 1 < n ? 2 * dm + 1 : n;
        C = reach > C ? reach : C;
    }
    int H = 0;
    for (int64_t v = C; v; v >>= 1) ++H;
    const int32_t* dmax_dev = nullptr;
    if (g_time_reassign_cwt_tables.get(dmax, (size_t)rows, &dmax_dev)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch_time_reassign_cwt<T>(W, Wd, rsc, dmax_dev, rot_lo, rot_hi, Tx, acc, peak, batch, rows, n, H, gamma,
                                           !(flags & SSQ_TSSQ_CWT_NO_WINDOW), as_stream(stream));
    });
}

}  // extern "C"
