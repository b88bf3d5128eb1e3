// ssq_reassign_cwt.inl -- ssq_reassign_cwt: the reassigned scalogram (Auger, Flandrin 1995) -- the energy of every point
// of a (batch, rows, n) CWT moves along BOTH axes, to the bin of its instantaneous frequency on the synchrosqueezing grid
// and to its group delay. The rule of the fixed-point scatter (ssq_fixed_scatter.inl: kernels, launcher, headroom) and
// the C-ABI entries; included by ssq_time_reassign.hip after ssq_reassign2d.inl, whose shift it takes. include/ssq_hip.h
// states what is computed; DESIGN.md section 4.5.10 the sizing.
//
// What differs from the STFT form is every index: the destination row is bin_from_w of the point's frequency (a log,
// log-piecewise or linear grid), the column shift is scaled by the row's scale, the displacement bound is per row, a row
// weight multiplies the term, and the rows of the LDS window are BINS: the window of a tile of TR x TC sources starts HR
// rows below the smallest home[i] of the tile's rows -- home[i] being where the caller expects the energy of row i to
// land -- and HC columns left of the tile. Integer addition is associative, so `home` (and the window itself) decides
// the speed and nothing else.
namespace ssq {

#include "ssq_point_math.inl"

template <typename T>
struct reassign_cwt_rule {
    static constexpr int TR = 8, TC = 256;      // sources of a tile: rows x columns (a column per work-item)
    static constexpr int HR = 4, HC = 64;       // the window's halo: bins below the smallest home and above it + TR; columns:
    static constexpr int WORDS = 1, CHUNK = 3;  // 16 x 384 cells = 48 KiB, three per CU; 3 lines of the write-out at a time
    static constexpr bool WEIGHTED = true;
    FixedPlanes<T> in;                          // W, dW, Wd
    const double *cst, *rsc;
    const int32_t *dmax, *home;
    SsqParams sp;

    static __device__ __forceinline__ int shift(unsigned long long peak_bits, int H) {
        return reassign2d_rule<T>::shift(peak_bits, H);
    }
    // below the smallest home of the tile's rows (any int32 will do: 64-bit from here on)
    __device__ __forceinline__ int64_t first_window_row(int64_t r0, unsigned rows) const {
        int32_t hmin = home[r0];
        for (int j = 1; j < TR && r0 + j < (int64_t)rows; ++j) hmin = home[r0 + j] < hmin ? home[r0 + j] : hmin;
        return (int64_t)hmin - HR;
    }
    template <typename ADD>
    __device__ __forceinline__ void place(const FixedPoint& p, double e, int64_t i, int64_t c, const FixedAt& at,
                                          ADD&& add) const {
        const int64_t omax = (int64_t)at.rows - 1;
        int64_t k2 = i;
        int d = 0;
        if (in.d) {
            const double w = fabs(phase_ratio(p.dr, p.di, p.gr, p.gi));         // |Im(dW / W)| / 2 pi
            k2 = bin_from_w(w, sp, omax);                                       // 0 .. rows - 1, whatever w is
            if (sp.flipud) k2 = omax - k2;
        }
        if (in.t) {
            const double s = (p.ti * p.gr - p.tr * p.gi) / e;                   // Im(Wd / W) = Re(T / W) / r
            const double dd = rint(s * rsc[i]);
            if (!(fabs(dd) <= (double)dmax[i])) return;                         // (NaN included)
            d = (int)dd;
        }
        const int64_t c2 = c + d;
        if (c2 < 0 || c2 >= (int64_t)at.n) return;
        add(k2, c2, {(unsigned long long)ldexp(e * cst[i], at.sh)});
    }
};

static DeviceTableCache g_reassign_cwt_tables;      // the rows' dmax

}  // namespace ssq

extern "C" {

int ssq_reassign_cwt_tile(int which) {
    using R = ssq::reassign_cwt_rule<float>;
    switch (which) {
        case 0: return R::TR;
        case 1: return R::TC;
        case 2: return R::HR;
        case 3: return R::HC;
        case 4: return (int)ssq::FXS_MAX_GRID;
        case 5: return R::TR + 2 * R::HR;
        case 6: return R::TC + 2 * R::HC;
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
    int64_t C = 0;
    int H = 0;
    if (fixed_headroom("ssq_reassign_cwt", time ? dmax : nullptr, 0, rows, n, freq, C, H)) return -1;
    SSQ_REQUIRE(C < ((int64_t)1 << 40), "ssq_reassign_cwt: %lld terms can meet in a cell, fewer than 2^40", (long long)C);
    const int32_t* dmax_dev = nullptr;
    if (time && g_reassign_cwt_tables.get(dmax, (size_t)rows, &dmax_dev)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const reassign_cwt_rule<T> rule{{(const T*)W, freq ? (const T*)dW : nullptr, time ? (const T*)Wd : nullptr},
                                        cst, rsc, dmax_dev, home, sp};
        return launch_fixed_scatter<T>(rule, gamma, Rx, acc, peak, batch, rows, n, H, window, as_stream(stream));
    });
}

}  // extern "C"
