// ssq_multi_squeeze.inl -- the kernel and the launcher of ssq_multi_squeeze, the multisynchrosqueezing transform (MSST;
// Yu, Wang, Zhao 2019): the first-order frequency map applied to its own output n_iter - 1 times, then the ordered
// accumulate. Included by ssq_kernels.hip inside `namespace ssq`, after the accumulate kernels whose pieces it uses
// (SideVal, point_bin; Term, FoldLower of ssq_reassign_dev.h), and compiled with that unit's -ffp-contract=off.
// include/ssq_hip.h states what is computed; DESIGN.md section 4.5.8 the sizing and what was measured.
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
constexpr int MSST_WC = 4, MSST_RL = 16;              // columns and row-lanes of a wavefront
constexpr int64_t MSST_MAX_ITER = 1024;
// reals of LDS per row and column: a complex Tx cell and a w
constexpr int MSST_REALS = 3;
template <typename T> constexpr int64_t msst_tile_rows(int cols) { return (int64_t)(LDS_CAP / ((size_t)cols * MSST_REALS * sizeof(T))); }

__device__ __forceinline__ bool msst_finite(double x) { return fabs(x) < (double)INFINITY; }     // (false for NaN)
__device__ __forceinline__ int msst_widx(int i, int c) { return MSST_WC * i + ((c + ((i >> 2) & 2)) & (MSST_WC - 1)); }

template <typename T, bool CST64, int TC>
__global__ __launch_bounds__(64 * (TC / MSST_WC)) void multi_squeeze_kernel(
    const T* __restrict__ Sx, const T* __restrict__ w, T* __restrict__ Tx, T* __restrict__ wf,
    const void* __restrict__ cst, SsqParams sp, double f0, double df, int rows, unsigned n, int n_iter, int interp) {
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
    const double pmax = (double)(rows - 1);

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
                    const double p = (f - f0) / df;
                    moving = p >= 0.0 && p <= pmax;                             // (false for NaN)
                    if (moving) {
                        double g = (double)wslab[msst_widx((int)rint(p), cl)];  // round half to even
                        if (interp) {
                            const int fl = (int)floor(p);
                            const int ia = fl < rows - 2 ? fl : rows - 2;
                            const double a = p - (double)ia;
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

// The widest tile whose rows fit the LDS (msst_tile_rows: 16, 8 or 4 columns), `batch` in launches of at most 65535
// signals (grid.y). The caller has checked rows <= msst_tile_rows<T>(4).
template <typename T, bool CST64>
static int launch_multi_squeeze(const void* Sx, const void* w, void* Tx, void* wf, const void* cst, const SsqParams& sp,
                                int64_t batch, int64_t rows, int64_t n, double f0, double df, int64_t n_iter, int interp,
                                hipStream_t stream) {
    auto launch = [&](auto tc) -> int {
        constexpr int TC = decltype(tc)::value;
        const size_t plane = (size_t)rows * (size_t)n;
        for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
            const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
            const int rc = launch_lds(multi_squeeze_kernel<T, CST64, TC>,
                                      dim3((unsigned)(((n + TC - 1) / TC + 7) / 8 * 8), (unsigned)nb), dim3(64 * (TC / MSST_WC)),
                                      (size_t)rows * TC * MSST_REALS * sizeof(T), stream, (const T*)Sx + 2 * b0 * plane,
                                      (const T*)w + b0 * plane, (T*)Tx + 2 * b0 * plane, wf ? (T*)wf + b0 * plane : (T*)nullptr,
                                      cst, sp, f0, df, (int)rows, (unsigned)n, (int)n_iter, interp);
            if (rc) return rc;
        }
        return 0;
    };
    if (rows <= msst_tile_rows<T>(16)) return launch(int_c<16>{});
    if (rows <= msst_tile_rows<T>(8)) return launch(int_c<8>{});
    return launch(int_c<4>{});
}
