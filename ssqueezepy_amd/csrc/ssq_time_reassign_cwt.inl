// ssq_time_reassign_cwt.inl -- ssq_time_reassign_cwt: the time-reassigned synchrosqueezed CWT -- every coefficient of a
// (batch, rows, n) CWT moves along its row to its group delay, rotated to the signal's origin first so that the terms
// that meet in a cell add coherently. The rule of the fixed-point scatter (ssq_fixed_scatter.inl: kernels, launcher,
// headroom) and the C-ABI entries; included by ssq_time_reassign.hip after ssq_reassign_cwt.inl. include/ssq_hip.h states
// what is computed; DESIGN.md section 4.5.12 the sizing.
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

template <typename T>
struct time_reassign_cwt_rule {
    // sources of a tile: rows x columns (a column per work-item, both rows in one pass: the scatter's row loop is one
    // step and requests nothing ahead)
    static constexpr int TR = 2, TC = 256;
    static constexpr int HR = 0, HC = 640;      // the window's halo in columns, on either side (no row halo: a point stays in its row):
    static constexpr int WORDS = 2, CHUNK = 3;  // 2 x 1536 cells of 16 bytes = 48 KiB: three per CU (the widest of the five
                                                // shapes measured and the fastest: profiles/tssq_cwt.txt); 3 lines at a time
    static constexpr bool WEIGHTED = false;
    static_assert(TR == FXS_RP, "a work-item per source of the tile: one pass");
    static_assert(TC == TCW_P, "a tile starts at a multiple of P: rot_hi is uniform over a tile's row");
    FixedPlanes<T> in;                          // W, none, Wd
    const double *rsc;
    const int32_t* dmax;
    const double *rot_lo, *rot_hi;

    // sh of a signal from its peak word (the bits of the largest kept |W|^2) and H = bit_length(terms a cell can receive):
    // a component of a term is below 2^hx (1 + a few ulp), hx = ceil(ex / 2)
    static __device__ __forceinline__ int shift(unsigned long long peak_bits, int H) {
        int ex = 0;
        (void)frexp(__builtin_bit_cast(double, peak_bits), &ex);
        return 61 - H - ((ex + 1) >> 1);                        // (an arithmetic shift: the ceiling for either sign)
    }
    __device__ __forceinline__ int64_t first_window_row(int64_t r0, unsigned) const { return r0; }
    template <typename ADD>
    __device__ __forceinline__ void place(const FixedPoint& p, double e, int64_t i, int64_t c, const FixedAt& at,
                                          ADD&& add) const {
        const double s = (p.ti * p.gr - p.tr * p.gi) / e;                       // Im(Wd / W) = Re(T / W) / r
        const double dd = rint(s * rsc[i]);
        if (!(fabs(dd) <= (double)dmax[i])) return;                             // (NaN included)
        const int64_t c2 = c + (int)dd;
        if (c2 < 0 || c2 >= (int64_t)at.n) return;
        double ur = 1., ui = 0.;
        if (rot_lo) {
            const size_t l = 2 * ((size_t)i * TCW_P + (size_t)at.col), h = 2 * ((size_t)i * at.ctiles + at.ct);
            const double lr = rot_lo[l], li = rot_lo[l + 1], hr = rot_hi[h], hi = rot_hi[h + 1];
            ur = hr * lr - hi * li; ui = hr * li + hi * lr;
        }
        const double zr = ur * p.gr - ui * p.gi, zi = ur * p.gi + ui * p.gr;
        // (|z| 2^sh < 2^62: the cast truncates toward zero; two's complement, so the sum may be taken unsigned)
        add(i, c2, {(unsigned long long)(long long)ldexp(zr, at.sh), (unsigned long long)(long long)ldexp(zi, at.sh)});
    }
};

static DeviceTableCache g_time_reassign_cwt_tables;     // the rows' dmax

}  // namespace ssq

extern "C" {

int ssq_time_reassign_cwt_tile(int which) {
    using R = ssq::time_reassign_cwt_rule<float>;
    switch (which) {
        case 0: return R::TR;
        case 1: return R::TC;
        case 2: return R::HC;
        case 3: return R::TC + 2 * R::HC;
        case 4: return (int)ssq::FXS_MAX_GRID;
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
    int64_t C = 0;
    int H = 0;
    if (fixed_headroom("ssq_time_reassign_cwt", dmax, 0, rows, n, false, C, H)) return -1;
    const int32_t* dmax_dev = nullptr;
    if (g_time_reassign_cwt_tables.get(dmax, (size_t)rows, &dmax_dev)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const time_reassign_cwt_rule<T> rule{{(const T*)W, nullptr, (const T*)Wd}, rsc, dmax_dev, (const double*)rot_lo,
                                             (const double*)rot_hi};
        return launch_fixed_scatter<T>(rule, gamma, Tx, acc, peak, batch, rows, n, H, !(flags & SSQ_TSSQ_CWT_NO_WINDOW),
                                       as_stream(stream));
    });
}

}  // extern "C"
