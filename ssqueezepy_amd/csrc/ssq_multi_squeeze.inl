// ssq_multi_squeeze.inl -- the kernel and the launcher of ssq_multi_squeeze and ssq_multi_squeeze_cwt, the
// multisynchrosqueezing transform (MSST; Yu, Wang, Zhao 2019): the first-order frequency map applied to its own output
// n_iter - 1 times, then the ordered accumulate. Included by ssq_kernels.hip inside `namespace ssq`, after the
// accumulate kernels whose pieces it uses (SideVal, point_bin; Term, FoldLower of ssq_reassign_dev.h), and compiled with
// that unit's -ffp-contract=off. include/ssq_hip.h states what is computed; DESIGN.md section 4.5.8 the sizing and what
// was measured, section 4.5.11 the same for the row table.
//
// The shape is accumulate_tile16_kernel's with 16 row-lanes: a wavefront owns 4 adjacent columns x 16 row-lanes
// (lane = 16 * column + row-lane), a workgroup is TC / 4 such wavefronts (TC = 16, 8 or 4 columns), the Tx slab of a
// wavefront is skewed in LDS, the 16 rows of a step are combined with FoldLower in ascending row order and the
// highest lane of a cell stores. New here:
//   * a second slab per wavefront holds its 4 columns of `w` (rows x 4 reals), so a row costs 3 reals of LDS per
//     column where the accumulate tile takes 2. The workgroup fills all its slabs in one pass over `w` -- a row of
//     the tile is one TC-column segment -- and synchronises once; from then on the wavefronts are on their own until
//     the write-out, as in the accumulate kernel.
//   * the slab's layout: (row i, column c) at 4 i + ((c + ((i >> 2) & 2)) & 3). A wavefront's first gather reads 16
//     adjacent rows of each column; LDS banks conflict inside a half-wave (2 columns x 16 rows) -- 32 banks of 4 bytes
//     for a 4-byte read, 64 for an 8-byte one --, where rows i and i + 8 of a column are 32 reals apart: the skew moves
//     the second eight rows by two columns, so the 32 lanes touch 32 different banks (float32) or 64 (float64).
//     Later gathers are wherever the map points; nothing can be laid out for them.
//   * the iteration: per lane a loop of LDS gathers in float64, left by the whole wavefront as soon as a ballot says
//     that no lane is still moving. Sx and the weight of the row batch that takes the slot next are requested before
//     the loop starts (the rolling prefetch of accumulate_tile16_kernel, depth 2), so they arrive under it.
//   * `wf`, when asked for, is written by the lane that walked the point.
//   * the position rule (POS): how a frequency becomes a place between two rows. The kernel asks it four things --
//     `find` (the place of `f`, false outside the rows' range), `nearest` (the row a place rounds to, half to even),
//     `lower` (the lower of the two rows around it, at most rows - 2) and `frac` (how far the place lies from that row
//     towards the next) -- and gives it the LDS behind the slabs (`ROW_BYTES` per row) to stage what it needs.
//     MsstLinearRows: rows at f0 + i df, the place is the real p = (f - f0) / df, no LDS. MsstTableRows: rows at
//     fr[i], a strictly monotone float64 table of either direction staged once per workgroup; the place is the
//     interval (i0, a), found from a closed-form guess where the table has one (MsstHint) and by a branch-free binary
//     search of ceil(log2(rows - 1)) dependent LDS reads where it has none or the guess is off by more than a row.
constexpr int MSST_WC = 4, MSST_RL = 16;              // columns and row-lanes of a wavefront
constexpr int64_t MSST_MAX_ITER = 1024;
// reals of LDS per row and column: a complex Tx cell and a w
constexpr int MSST_REALS = 3;
// the most rows of a tile of `cols` columns; `row_bytes`: what the position rule keeps per row on top of the slabs
template <typename T> constexpr int64_t msst_tile_rows(int cols, int row_bytes = 0) {
    return (int64_t)(LDS_CAP / ((size_t)cols * MSST_REALS * sizeof(T) + (size_t)row_bytes));
}

__device__ __forceinline__ bool msst_finite(double x) { return fabs(x) < (double)INFINITY; }     // (false for NaN)
__device__ __forceinline__ int msst_widx(int i, int c) { return MSST_WC * i + ((c + ((i >> 2) & 2)) & (MSST_WC - 1)); }

// row i sits at f0 + i df
struct MsstLinearRows {
    static constexpr int ROW_BYTES = 0;
    using place_t = double;
    double f0, df;
    __device__ __forceinline__ void stage(unsigned char*, int, int, int) {}
    __device__ __forceinline__ bool find(double f, int rows, place_t& p) const {
        const double pmax = (double)(rows - 1);
        p = (f - f0) / df;
        return p >= 0.0 && p <= pmax;                                           // (false for NaN)
    }
    __device__ __forceinline__ int nearest(const place_t& p) const { return (int)rint(p); }     // round half to even
    __device__ __forceinline__ int lower(const place_t& p, int rows) const {
        const int fl = (int)floor(p);
        return fl < rows - 2 ? fl : rows - 2;
    }
    __device__ __forceinline__ double frac(const place_t& p, int ia) const { return p - (double)ia; }
};

// A closed-form first guess of a table row, for tables that are geometric in one or two pieces ('log' and
// 'log-piecewise' scales): row ~ row0[p] + (log2f(f) - l0[p]) * slope[p], p the piece on f's side of `seam`. The entry
// fits it to the host table and keeps it only if it names a row within one of the right one at every row's frequency
// and between every two rows (msst_fit_hint); `pieces` = 0 turns it off. float32 throughout: the guess is checked
// against the table, so it can cost time and never a bit.
struct MsstHint {
    int pieces;
    double seam;
    float l0[2], slope[2], row0[2];
    __host__ __device__ __forceinline__ int guess(double f, bool desc, int rows) const {
        const int p = (desc ? f >= seam : f <= seam) ? 0 : 1;
        const float pos = row0[p] + (log2f((float)f) - l0[p]) * slope[p];
        return (int)fminf(fmaxf(floorf(pos), 0.0f), (float)(rows - 2));         // (a NaN becomes row 0)
    }
};

// row i sits at fr[i]: `fr` (rows,) float64 on the device, finite and strictly monotone (the entry has checked the host
// copy); `lo`, `hi` its smaller and larger end, `desc` whether it descends. The table is staged behind the slabs by the
// whole workgroup before the barrier that publishes the w slabs.
struct MsstTableRows {
    static constexpr int ROW_BYTES = 8;
    struct place_t { int i0; double a; };
    const double* fr;
    double lo, hi;
    int desc;
    MsstHint hint;
    const double* tab;
    __device__ __forceinline__ void stage(unsigned char* lds, int rows, int tid, int nth) {
        double* t = reinterpret_cast<double*>(lds);
        for (int i = tid; i < rows; i += nth) t[i] = fr[i];
        tab = t;
    }
    // whether a row at `t` lies at or before `f` in the table's direction
    __device__ __forceinline__ bool before(double t, double f) const { return desc ? t >= f : t <= f; }
    // i0: the largest i <= rows - 2 whose row lies at or before `f`. Row 0 always does for an `f` inside the range, and
    // the rows that do are a prefix. With a hint: the guessed row g is i0 if it lies before `f` and the next one does not
    // (or there is no next interval) -- two independent reads, the two the interpolation needs anyway --, g - 1 or g + 1
    // take one read more; anything else goes to the search. The search halves [base, base + len) keeping `base` a row
    // that lies before `f`: ceil(log2(rows - 1)) dependent reads, the same number for every lane.
    __device__ __forceinline__ bool find(double f, int rows, place_t& p) const {
        if (!(f >= lo && f <= hi)) return false;                                // (false for NaN)
        int base = -1;
        if (hint.pieces) {
            const int g = hint.guess(f, desc != 0, rows);
            const bool b0 = before(tab[g], f), b1 = before(tab[g + 1], f);
            if (b0 && (g == rows - 2 || !b1)) base = g;
            else if (!b0) { if (g > 0 && before(tab[g - 1], f)) base = g - 1; }
            else if (g + 1 == rows - 2 || !before(tab[g + 2], f)) base = g + 1;     // (here g < rows - 2)
        }
        if (base < 0) {
            base = 0;
            for (int len = rows - 1; len > 1;) {
                const int half = len >> 1;
                base = before(tab[base + half], f) ? base + half : base;
                len -= half;
            }
        }
        const double t0 = tab[base], t1 = tab[base + 1];
        p.i0 = base;
        p.a = (f - t0) / (t1 - t0);
        return true;
    }
    __device__ __forceinline__ int nearest(const place_t& p) const {            // half to the even row
        return p.i0 + (int)(p.a > 0.5 || (p.a == 0.5 && (p.i0 & 1)));
    }
    __device__ __forceinline__ int lower(const place_t& p, int) const { return p.i0; }
    __device__ __forceinline__ double frac(const place_t& p, int) const { return p.a; }
};

// The hint of a host table, or one with `pieces` = 0: two geometric pieces that meet at the row where log2(fr) bends
// most, each through its end rows (one geometric table is two pieces of one slope), kept if the guess is within one
// row of the right one at every row's frequency and at the geometric mean of every two neighbours -- then it is off by
// at most two anywhere, and MsstTableRows::find corrects one and searches for the rest.
static MsstHint msst_fit_hint(const double* fr, int64_t rows) {
    MsstHint h{};
    if (rows < 4) return h;
    for (int64_t i = 0; i < rows; ++i)
        if (!(fr[i] > 0.0)) return h;
    std::vector<double> lg((size_t)rows);
    for (int64_t i = 0; i < rows; ++i) lg[(size_t)i] = log2(fr[i]);
    int64_t s = 1;
    double bend = -1.0;
    for (int64_t i = 1; i + 1 < rows; ++i) {
        const double d2 = fabs(lg[(size_t)i + 1] - 2.0 * lg[(size_t)i] + lg[(size_t)i - 1]);
        if (d2 > bend) { bend = d2; s = i; }
    }
    const bool desc = fr[1] < fr[0];
    h.seam = fr[s];
    h.l0[0] = (float)lg[0]; h.row0[0] = 0.0f;
    h.slope[0] = (float)((double)s / (lg[(size_t)s] - lg[0]));
    h.l0[1] = (float)lg[(size_t)s]; h.row0[1] = (float)s;
    h.slope[1] = (float)((double)(rows - 1 - s) / (lg[(size_t)rows - 1] - lg[(size_t)s]));
    for (int64_t i = 0; i + 1 < rows; ++i)
        for (double f : {fr[i], sqrt(fr[i] * fr[i + 1])}) {
            const int64_t g = h.guess(f, desc, (int)rows);
            if (g < i - 1 || g > i + 1) return h;                               // (pieces is still 0)
        }
    h.pieces = 2;
    return h;
}

template <typename T, bool CST64, int TC, typename POS>
__global__ __launch_bounds__(64 * (TC / MSST_WC)) void multi_squeeze_kernel(
    const T* __restrict__ Sx, const T* __restrict__ w, T* __restrict__ Tx, T* __restrict__ wf,
    const void* __restrict__ cst, SsqParams sp, POS pos, int rows, unsigned n, int n_iter, int interp) {
    constexpr int WC = MSST_WC, RL = MSST_RL, U = 2;
    constexpr int NTH = 64 * (TC / WC);
    using TM = Term<T, CST64>;
    using term_t = typename TM::type;
    using w_t = typename TM::wtype;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* tile = reinterpret_cast<T*>(lds_raw);                        // [TC / 4 waves][rows][4][2], cells skewed
    T* wtile = tile + (size_t)rows * TC * 2;                        // [TC / 4 waves][rows][4], see msst_widx
    T* slab = tile + (size_t)wave * rows * WC * 2;
    const T* wslab = wtile + (size_t)wave * rows * WC;
    const int cl = lane / RL, rl = lane % RL;

    // XCD-aware tile order, as accumulate_tile16_kernel (grid.x is a multiple of 8)
    const unsigned per = gridDim.x >> 3;
    const unsigned tile_id = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if ((uint64_t)tile_id * TC >= n) return;
    const unsigned j = tile_id * TC + wave * WC + cl;               // (n + TC < 2^32: rows >= 2 and rows n < 2^32)
    const bool col_ok = j < n;
    const int64_t omax = rows - 1;
    const size_t boff = (size_t)blockIdx.y * (size_t)rows * (size_t)n;
    const T* Sb = Sx + 2 * boff;
    const T* wb = w + boff;
    T* Tb = Tx + 2 * boff;
    T* fb = wf ? wf + boff : nullptr;

    for (int t = lane; t < rows * WC * 2; t += 64) slab[t] = T(0);
    {
        const int cc = threadIdx.x % TC, rr = threadIdx.x / TC;
        const unsigned jj = tile_id * TC + cc;
        T* ws = wtile + (size_t)(cc / WC) * rows * WC;
        if (jj < n)
            for (int i = rr; i < rows; i += NTH / TC) ws[msst_widx(i, cc % WC)] = wb[(size_t)((unsigned)i * n + jj)];
    }
    pos.stage(reinterpret_cast<unsigned char*>(wtile + (size_t)rows * TC), rows, (int)threadIdx.x, NTH);
    __syncthreads();

    // rolling prefetch of Sx and the weights: slot u holds rows i0 + 16 u + rl; loads unconditional (clamped)
    T zc[U], zd[U];
    w_t wt[U];
    const unsigned jc = col_ok ? j : n - 1;
    auto request = [&](int u, int i) {
        const int ic = i < rows ? i : rows - 1;
        const size_t q = (size_t)((unsigned)ic * n + jc);
        zc[u] = Sb[2 * q];
        zd[u] = Sb[2 * q + 1];
        wt[u] = ((const w_t*)cst)[ic];
    };
#pragma unroll
    for (int u = 0; u < U; ++u) request(u, u * RL + rl);

    for (int i0 = 0; i0 < rows; i0 += RL * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * RL + rl;
            const bool live = col_ok && i < rows;
            const T c_re = zc[u], c_im = zd[u];
            const w_t wsel = wt[u];
            request(u, i + RL * U);                       // the slot's next rows: they arrive under the iteration
            double f = (double)INFINITY;
            if (live) f = (double)wslab[msst_widx(i, cl)];
            const bool have = msst_finite(f);
            bool moving = have;
            for (int it = 1; it < n_iter; ++it) {
                if (!__builtin_amdgcn_ballot_w64(moving)) break;                // wave-uniform
                if (moving) {
                    typename POS::place_t p;
                    moving = pos.find(f, rows, p);
                    if (moving) {
                        double g = (double)wslab[msst_widx(pos.nearest(p), cl)];
                        if (interp) {
                            const int ia = pos.lower(p, rows);
                            const double a = pos.frac(p, ia);
                            const double wa = (double)wslab[msst_widx(ia, cl)], wc = (double)wslab[msst_widx(ia + 1, cl)];
                            if (msst_finite(wa) && msst_finite(wc)) g = wa + a * (wc - wa);
                        }
                        moving = msst_finite(g) && g != f;
                        if (msst_finite(g)) f = g;
                    }
                }
            }
            SideVal<T, BIN_FROM_W> sv;
            sv.w = have ? (T)f : (T)INFINITY;
            int k = -1;
            if (live) {
                if (fb) fb[(size_t)((unsigned)i * n + j)] = sv.w;
                k = (int)point_bin<T, BIN_FROM_W, false>(c_re, c_im, sv, i, nullptr, sp, omax);
            }
            term_t tr = term_t(0), ti = term_t(0);
            T ore = T(0), oim = T(0);
            T* cell = slab;
            if (k >= 0) {
                tr = TM::make(c_re, wsel);
                ti = TM::make(c_im, wsel);
                cell = slab + 2 * (k * WC + ((cl + k) & (WC - 1)));
                ore = cell[0]; oim = cell[1];
            }
            unsigned long long higher = 0;
            const int key = k + 1;
            FoldLower<RL - 1, false, TM, T, term_t>::run(key, __builtin_amdgcn_ballot_w64(key != 0), tr, ti, ore, oim, higher);
            ore = TM::fold(ore, tr); oim = TM::fold(oim, ti);
            const bool last = !((higher >> lane) & 1ull);
            if (k >= 0 && last) { cell[0] = ore; cell[1] = oim; }
            __builtin_amdgcn_wave_barrier();
        }
    }
    // write-out by the whole workgroup, a TC-column segment per row
    __syncthreads();
    {
        const int cc = threadIdx.x % TC, rr = threadIdx.x / TC;
        const unsigned jj = tile_id * TC + cc;
        const T* ws = tile + (size_t)(cc / WC) * rows * WC * 2;
        const int c4 = cc % WC;
        if (jj < n) {
#pragma unroll 4
            for (int k = rr; k < rows; k += NTH / TC) {
                const T* cell = ws + 2 * (k * WC + ((c4 + k) & (WC - 1)));
                const size_t q = (size_t)((unsigned)k * n + jj);
                Tb[2 * q] = cell[0];
                Tb[2 * q + 1] = cell[1];
            }
        }
    }
}

// The columns of the widest tile whose rows fit the LDS (msst_tile_rows: 16, 8 or 4), 0 where none does
template <typename T, typename POS>
static int msst_tile_cols(int64_t rows) {
    for (int cols : {16, 8, 4})
        if (rows <= msst_tile_rows<T>(cols, POS::ROW_BYTES)) return cols;
    return 0;
}

// The widest tile that fits, `batch` in launches of at most 65535 signals (grid.y). The caller has checked
// rows <= msst_tile_rows<T>(4, POS::ROW_BYTES).
template <typename T, bool CST64, typename POS>
static int launch_multi_squeeze(const void* Sx, const void* w, void* Tx, void* wf, const void* cst, const SsqParams& sp,
                                int64_t batch, int64_t rows, int64_t n, const POS& pos, int64_t n_iter, int interp,
                                hipStream_t stream) {
    auto launch = [&](auto tc) -> int {
        constexpr int TC = decltype(tc)::value;
        const size_t plane = (size_t)rows * (size_t)n;
        for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
            const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
            const int rc = launch_lds(multi_squeeze_kernel<T, CST64, TC, POS>,
                                      dim3((unsigned)(((n + TC - 1) / TC + 7) / 8 * 8), (unsigned)nb), dim3(64 * (TC / MSST_WC)),
                                      (size_t)rows * (TC * MSST_REALS * sizeof(T) + POS::ROW_BYTES), stream,
                                      (const T*)Sx + 2 * b0 * plane, (const T*)w + b0 * plane, (T*)Tx + 2 * b0 * plane,
                                      wf ? (T*)wf + b0 * plane : (T*)nullptr, cst, sp, pos, (int)rows, (unsigned)n,
                                      (int)n_iter, interp);
            if (rc) return rc;
        }
        return 0;
    };
    const int cols = msst_tile_cols<T, POS>(rows);
    if (cols == 16) return launch(int_c<16>{});
    if (cols == 8) return launch(int_c<8>{});
    return launch(int_c<4>{});
}
