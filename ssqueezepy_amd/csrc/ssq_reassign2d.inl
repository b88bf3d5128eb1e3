// ssq_reassign2d.inl -- ssq_reassign2d: the reassigned spectrogram (Kodera, Gendrin, de Villedary 1978; Auger, Flandrin
// 1995) -- the energy of every point of a (batch, rows, n) plane moves along BOTH axes, to its instantaneous frequency
// and its group delay. The rule of the fixed-point scatter (ssq_fixed_scatter.inl: kernels, launcher, headroom) and the
// C-ABI entries; included by ssq_time_reassign.hip after that file. include/ssq_hip.h states what is computed; DESIGN.md
// section 4.5.9 the sizing.
//
// A term is the energy of a point; its destination is m rows and d columns from the point, reflected at row 0; the LDS
// window of a tile lies around the tile itself, HR rows and HC columns wider on every side.
namespace ssq {

constexpr double R2D_TWO_PI = 6.283185307179586;

// (the rules are named as the entries are: a kernel's name carries its rule's, and tools/isa_report.py filters by it)
template <typename T>
struct reassign2d_rule {
    static constexpr int TR = 8, TC = 256;      // sources of a tile: rows x columns (a column per work-item)
    static constexpr int HR = 2, HC = 64;       // the window's halo: rows above and below, columns left and right:
    static constexpr int WORDS = 1, CHUNK = 3;  // 12 x 384 cells = 36 KiB; a wavefront holds 3 of its lines at a time
    static constexpr bool WEIGHTED = false;
    FixedPlanes<T> in;                          // Sx, dSx, Vtg
    double df, cps;
    int64_t kmax;
    int dmax;

    // sh of a signal from its peak word (the bits of the largest kept energy) and H = bit_length(terms a cell can receive)
    static __device__ __forceinline__ int shift(unsigned long long peak_bits, int H) {
        int ex = 0;
        (void)frexp(__builtin_bit_cast(double, peak_bits), &ex);
        return 62 - H - ex;
    }
    __device__ __forceinline__ int64_t first_window_row(int64_t r0, unsigned) const { return r0 - HR; }
    template <typename ADD>
    __device__ __forceinline__ void place(const FixedPoint& p, double e, int64_t k, int64_t c, const FixedAt& at,
                                          ADD&& add) const {
        int64_t m = 0;
        int d = 0;
        if (in.d) {
            const double im = (p.di * p.gr - p.dr * p.gi) / e;                  // Im(dSx / Sx)
            const double mf = rint(((-im) / R2D_TWO_PI) / df);
            if (!(fabs(mf) <= (double)kmax)) return;                            // (NaN included)
            m = (int64_t)mf;
        }
        if (in.t) {
            const double s = (p.tr * p.gr + p.ti * p.gi) / e;                   // Re(Vtg / Sx)
            const double dd = rint(s * cps);
            if (!(fabs(dd) <= (double)dmax)) return;
            d = (int)dd;
        }
        int64_t k2 = k + m;
        k2 = k2 < 0 ? -k2 : k2;
        const int64_t c2 = c + d;
        if (k2 > (int64_t)at.rows - 1 || c2 < 0 || c2 >= (int64_t)at.n) return;
        add(k2, c2, {(unsigned long long)ldexp(e, at.sh)});
    }
};

}  // namespace ssq

extern "C" {

int ssq_reassign2d_tile(int which) {
    using R = ssq::reassign2d_rule<float>;
    switch (which) {
        case 0: return R::TR;
        case 1: return R::TC;
        case 2: return R::HR;
        case 3: return R::HC;
        case 4: return (int)ssq::FXS_MAX_GRID;
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
    int64_t cell_terms = 0;
    int H = 0;
    if (fixed_headroom("ssq_reassign2d", nullptr, dmax, rows, n, true, cell_terms, H)) return -1;
    SSQ_REQUIRE(cell_terms < ((int64_t)1 << 40), "ssq_reassign2d: %lld rows x %lld columns can meet in a cell, fewer than 2^40",
                (long long)rows, (long long)(cell_terms / rows));
    // |k + m| <= rows - 1 needs |m| <= 2 (rows - 1): a larger kmax changes nothing and m stays below 2^33 (the kernel's
    // row arithmetic is 64-bit)
    const int64_t km = kmax < 2 * rows ? kmax : 2 * rows;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const reassign2d_rule<T> rule{{(const T*)Sx, freq ? (const T*)dSx : nullptr, dmax ? (const T*)Vtg : nullptr},
                                      fs / (double)n_fft, cols_per_second, km, (int)dmax};
        return launch_fixed_scatter<T>(rule, gamma, Rx, acc, peak, batch, rows, n, H, !(flags & SSQ_REASSIGN2D_NO_WINDOW),
                                       as_stream(stream));
    });
}

}  // extern "C"
