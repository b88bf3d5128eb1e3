// ssq_tile_dev.h -- device-side pieces shared by the three column-tile kernels of the fused ssq_cwt form
// (ssq_tile_ordered.hip: the ticketed float32 tile; ssq_tile_f64.hip / ssq_tile_pair.hip: the float64 tile with
// unordered adds, one / two columns per lane). Include inside namespace ssq, after ssq_point_math.inl. The term of a
// point and its fold into a cell (Term) come from ssq_reassign_dev.h.
#pragma once

constexpr int TILE_W = 8;         // taps
constexpr int TILE_NOBIN = 0xFFFF;

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    ssq_f2 av, bv, dv;
    av.x = a.x; av.y = a.y; bv.x = b.x; bv.y = b.y;
    SSQ_CMUL_PK(dv, av, bv);
    return make_float2(dv.x, dv.y);
}

// bin of a point the float32 screens could not decide (flipped as Tx wants it), or -1 when it
// does not contribute: the exact double sequence of the CPU path (~0.05 % of the points). Inline:
// a call would put the parameters on the stack and make the compiler wait for every load in
// flight at the join.
__device__ __forceinline__ int exact_bin(float2 W, float2 D, const SsqParams& sp, int omax, double gamma) {
    if (!(mag_of(W.x, W.y) > gamma)) return -1;
    const int ke = (int)bin_of_point_exact(D.x, D.y, W.x, W.y, sp, (int64_t)omax);
    return sp.flipud ? omax - ke : ke;
}

// Some pieces below are macros, expanded in the kernel's body: written as inline functions, the same arithmetic
// compiles to other instructions in some of the kernels (the compiler simplifies a callee on its own before
// inlining it, and the kernels are tuned to their instruction order; measured).
//
// TILE_BIN_SCREEN: the float32 screen of a point's bin from (Wx, dWx) = (W, V), as the block kernels' lean
// epilogue (emit_point<LEAN>): above / below the gamma band (m2hi, m2lo), ok (the screens decided), kf (the bin,
// flipped as Tx wants it). The kernel then takes kf when above and live, and asks exact_bin for the live points with
// !(below | (above & ok)). Uses sp, omax, fx, fa, m2hi, m2lo of the kernel.
#define TILE_BIN_SCREEN(GRID, W, V)                                                                            \
    const float cc = (W).x, dd = (W).y, aa = (V).x, bb = (V).y;                                               \
    const float m2 = cc * cc + dd * dd, num = bb * cc - aa * dd;                                              \
    const bool above = m2 > m2hi, below = m2 < m2lo;                                                          \
    const float w32 = fabsf(num * __builtin_amdgcn_rcpf(m2 * 6.2831855f));                                    \
    bool ok;                                                                                                  \
    const int kb = bin_screen_cwt<GRID>(w32, sp, omax, ok);                                                   \
    const int kf = (kb ^ fx) + fa

// tile3_kernel's form of it, per column: the bin, or -1; `pend`: a live point the screens could not decide
template <int GRID>
__device__ __forceinline__ int screened_bin(const ssq_f2 W, const ssq_f2 V, bool live, float m2hi, float m2lo,
                                            const SsqParams& sp, int omax, int fx, int fa, bool& pend) {
    TILE_BIN_SCREEN(GRID, W, V);
    pend = live && !(below | (above & ok));
    return (above && live) ? kf : -1;
}

// TILE_BPERMUTE8: the eight taps of a lane's point -- (ur, ui), the bits of a sample, from the lanes baddr / 4 + 0 ..
// 7 (the lanes hold a window of consecutive samples) into fr[0 .. 7], fi[0 .. 7] by ds_bpermute -- waited for
#define TILE_BPERMUTE8(fr, fi, baddr, ur, ui)                                                                  \
    do {                                                                                                      \
        SSQ_BPERMUTE_OFF(fr[0], baddr, ur, 0);  SSQ_BPERMUTE_OFF(fi[0], baddr, ui, 0);                        \
        SSQ_BPERMUTE_OFF(fr[1], baddr, ur, 4);  SSQ_BPERMUTE_OFF(fi[1], baddr, ui, 4);                        \
        SSQ_BPERMUTE_OFF(fr[2], baddr, ur, 8);  SSQ_BPERMUTE_OFF(fi[2], baddr, ui, 8);                        \
        SSQ_BPERMUTE_OFF(fr[3], baddr, ur, 12); SSQ_BPERMUTE_OFF(fi[3], baddr, ui, 12);                       \
        SSQ_BPERMUTE_OFF(fr[4], baddr, ur, 16); SSQ_BPERMUTE_OFF(fi[4], baddr, ui, 16);                       \
        SSQ_BPERMUTE_OFF(fr[5], baddr, ur, 20); SSQ_BPERMUTE_OFF(fi[5], baddr, ui, 20);                       \
        SSQ_BPERMUTE_OFF(fr[6], baddr, ur, 24); SSQ_BPERMUTE_OFF(fi[6], baddr, ui, 24);                       \
        SSQ_BPERMUTE_OFF(fr[7], baddr, ur, 28); SSQ_BPERMUTE_OFF(fi[7], baddr, ui, 28);                       \
        SSQ_LDS_WAIT();                                                                                       \
    } while (0)

// tile2_kernel's and tile3_kernel's form of it: the taps as (re, im) pairs
__device__ __forceinline__ void gather8(ssq_f2 (&sv)[TILE_W], int baddr, float ux, float uy) {
    int fr[TILE_W], fi[TILE_W];
    const int ur = __float_as_int(ux), ui = __float_as_int(uy);
    TILE_BPERMUTE8(fr, fi, baddr, ur, ui);
#pragma unroll
    for (int t = 0; t < TILE_W; ++t) { sv[t].x = __int_as_float(fr[t]); sv[t].y = __int_as_float(fi[t]); }
}

// Workgroup b runs on XCD b mod 8 (each XCD has its own L2). When `permute`, the workgroup's FIRST tile is permuted so
// that the 32 workgroups of an XCD walk 32 ADJACENT tiles at a time: neighbouring tiles read overlapping windows of
// the decimated samples (8 taps of halo; for R >= 64 the very same samples), which then meet in one L2 instead of
// being fetched from HBM once per tile. The stride between a workgroup's tiles stays G, so the lanes' weight phase is
// kept. (permute: the caller's test -- G a multiple of 8 and the permutation wanted -- written out at the call
// site, in the order that kernel was tuned with.)
#define TILE_FIRST_IF(permute, G) \
    ((permute) ? ((int)blockIdx.x & 7) * ((G) >> 3) + ((int)blockIdx.x >> 3) : (int)blockIdx.x)

// ---- The walk of tile2_kernel and tile3_kernel over the tiles, written once. Workgroup b walks tiles b, b + G, ...
// (b permuted per XCD, TILE_FIRST_IF) -- of each signal (then a signal's last round is short for the workgroups past
// ntx mod G, launch after launch: 304 against 320 tiles at config 2), or, A.carry, of the signals laid end to end
// (the launcher allows it when the lanes' weights survive the boundary). Tile t = columns COLS t - sh .. COLS t - sh
// + COLS - 1 of a signal: tile3_kernel's tiles start a column early when the left padding n1 is odd (sh = 1),
// tile2_kernel passes sh = 0; n1e = n1 - sh.
// Macros (see above): as inline functions or a struct, the walk compiled to other instructions in both kernels.
//
// TILE_WALK_TILES: the workgroup's tiles -- ntx per signal, the grid G, its first tile bid, per_sig per signal, ntl in
// all. Uses N (int64_t) and A (TileWalkArgs) of the kernel.
#define TILE_WALK_TILES(COLS, sh)                                                                              \
    const int ntx = (int)((N + (sh) + (COLS) - 1) / (COLS));                                                  \
    const int G = (int)gridDim.x;                                                                             \
    const int bid = TILE_FIRST_IF(A.xcd && (G & 7) == 0, G);                                                  \
    const int per_sig = bid < ntx ? (ntx - bid + G - 1) / G : 0;                                              \
    const int ntl = A.carry ? (int)(((int64_t)A.nsig * ntx - bid + G - 1) / G) : per_sig * A.nsig
// TILE_WALK_FINISH_ONLY: a wavefront without items (more wavefronts than items) takes part in the write-outs of the
// workgroup's tiles only: finish_tile(tile, signal) for each
#define TILE_WALK_FINISH_ONLY(finish_tile)                                                                     \
    do {                                                                                                      \
        int tx = bid, sg = 0;                                                                                 \
        for (int j = 0; j < ntl; ++j) {                                                                       \
            finish_tile(tx, sg);                                                                              \
            tx += G;                                                                                          \
            if (tx >= ntx) { tx = A.carry ? tx - ntx : bid; ++sg; }                                           \
        }                                                                                                     \
    } while (0)
// TILE_WALK_CURSORS: a wavefront's sequence of (tile, item) positions is walked by cursors, each an item index and
// the tile as the kernel uses it (Pos): n of the tile's first column (n1e + COLS t), the signal, and the byte offset
// of (signal, row 0, first column) in Wx -- moved by constants when the cursor's item index wraps (no 64-bit
// products, and no position records copied around per item). Declares Pos and next_tile(q): the tile after q, or
// q itself after the last. Uses N, na and A of the kernel.
#define TILE_WALK_CURSORS(COLS, n1e)                                                                       \
    struct Pos { int nabs0, sg; int64_t off8; };                                                              \
    const int nabs_step = G * (COLS), nabs_first = (n1e) + bid * (COLS), nabs_last = (n1e) + (ntx - 1) * (COLS); \
    const int64_t off8_step = (int64_t)G * (COLS) * 8;                                                        \
    /* (a signal's end: back to the workgroup's first tile, or -- carry -- on by the same stride into the next one) */ \
    const int64_t off8_wrap = A.carry ? ((int64_t)na * N + (int64_t)(G - ntx) * (COLS)) * 8                   \
                                      : ((int64_t)na * N - (int64_t)(per_sig - 1) * G * (COLS)) * 8;          \
    const int nabs_back = ntx * (COLS);                                                                       \
    auto next_tile = [&](Pos q) {                                                                             \
        Pos r = q;                                                                                            \
        r.nabs0 += nabs_step;                                                                                 \
        const bool wrap = r.nabs0 > nabs_last;                                                                \
        r.off8 += wrap ? off8_wrap : off8_step;                                                               \
        if (wrap) { r.nabs0 = A.carry ? r.nabs0 - nabs_back : nabs_first; ++r.sg; }                           \
        return (wrap && r.sg >= A.nsig) ? q : r;                /* (the tile after the last: the last) */     \
    }
// TILE_WALK_FIRST: cursor p on the workgroup's first tile
#define TILE_WALK_FIRST(p, COLS, sh) \
    do { (p).nabs0 = nabs_first; (p).sg = 0; (p).off8 = ((int64_t)bid * (COLS) - (sh)) * 8; } while (0)

// a finished tile: counted (what actually ran)
__device__ __forceinline__ void tile_count(unsigned long long* counters) {
    if (threadIdx.x == 0 && counters)
        __scoped_atomic_fetch_add(counters, 1ull, __ATOMIC_RELAXED, __MEMORY_SCOPE_DEVICE);
}
