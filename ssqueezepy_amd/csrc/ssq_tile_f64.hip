// ssq_tile_f64.hip -- the default column-tile kernel of the fused ssq_cwt form (float32 data, gfx950): `tile2_kernel`,
// a float64 Tx tile in LDS with unordered ds_add_f64. Interpolates Wx (and dWx) of most rows from decimated baseband
// samples (ssq_tile_fft.hip; math and planning: ssqueezepy_amd/_tiles.py), reads the other rows' Wx + bin back, and
// reassigns all of them -- replaces the reference's cwt + phase_cwt + ssqueeze loop nests for these rows
// (ssqueezepy/_cwt.py:167-177, algos.py:859-953).
//
// Compiled with -ffp-contract=off (bin indices); multiply-adds that may fuse are written as explicit fmaf so every
// instantiation rounds identically. The tuning switches of rounds 3-5 (ablation builds, shader-clock stamps) are not
// in this file: tools/r5/tile_switches.diff re-applies them.
//
// tile2_kernel (round 4): the work of the ticketed kernel (ssq_tile_ordered.hip) without its ticket chain.
//
// What round 4 measured on the MI355X (profiles/r4_ab_history.txt): the ticketed kernel
// spends a quarter of every tile at its boundary and is otherwise paced by the hand-overs (177 us
// of chain alone, 230 us of arithmetic alone, 256 us together); its time does not change when
// the gather, the modulation or the bin arithmetic are taken out, it is the same on 64 and on 256
// CUs (per tile), and LDS *float32* atomics, the obvious way around the tickets, take 193 cycles
// per wavefront instruction -- while ds_add_f64 takes 13.6 and ds_add_u64 10.8
// (tools/probes/lds_rmw_probe.hip).
//
// So the tile is kept in float64 and every wavefront adds its terms as soon as it has them
// (ds_add_f64, no return value): 16 bytes per cell, hence COLS = 32 columns per tile (16 when
// na > 319) and 64 / COLS consecutive rows per wavefront instruction (lane = sub-row h x column).
// Nothing orders the wavefronts inside a tile, so
//   * a wavefront owns a CONTIGUOUS block of the tile's rows (cost-balanced by the host), the
//     same block for every tile: consecutive rows share their decimation class, and the
//     interpolation weights of a class depend on the column only through n mod R -- the same
//     for every tile of a persistent workgroup whose tile stride (gridDim x COLS columns) is a
//     multiple of R: weights are re-read at class changes only, not per step;
//   * an item (= one wavefront instruction's rows) carries 16 bytes of state (one packed
//     record), the pipeline is: record two items ahead, samples one item ahead;
//   * a tile ends with two hardware barriers (all terms in / tile written out and cleared)
//     instead of 76 hand-overs.
// The sum of a cell is the float64 sum of its float32 (or float64) terms, rounded once: it
// differs from the reference's running float32 sum (algos.py:912-924) by that sum's own
// rounding, ~1e-7 of the largest cell (tests bound it at 1e-6); the bins are the same integers.
// float64 addition is not associative either, but with 300 terms of 24-bit mantissas the
// double sum's own rounding error is ~1e-16 relative: the float32 result differs between two
// arrival orders only when the exact sum lies within that of a float32 rounding boundary.
#include "ssq_common.h"
#include "ssq_reassign_dev.h"
#include "ssq_tiles.h"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace ssq {

#include "ssq_point_math.inl"
#include "ssq_tile_dev.h"

// Both tile kernels are bound by the instructions they issue, of every kind (round 4,
// profiles/r4_ab_history.txt: one instruction per cycle and CU; 210 per 64 points in the ticketed
// kernel). This one is built to issue few:
//   * an item (64 / COLS consecutive rows x COLS columns) has ONE scalar record (s_load through the
//     constant address space: the index is wavefront-uniform): the sub-rows are consecutive rows of
//     one class, so a lane's addresses are scalar bases + per-lane constants;
//   * one load of samples (or Wx + bin for rows read back) and one store of Wx per item, one
//     8-byte-per-lane store of Tx per 2 (4) rows x COLS columns of a finished tile;
//   * the interpolation weights stay in registers for the whole launch: a wavefront's block of
//     rows spans at most two decimation classes (the host cuts the blocks that way), and a lane's
//     weights depend on its column only through n mod R, the same for every tile of a workgroup
//     whose tile stride is a multiple of R (the launcher picks the grid that way).
// STORE_K (diagnostic builds, ssq_cwt_plan_set_bin_dump): every point's bin index goes to A.kdump as the
// reassignment consumes it -- what pins the kernel's index work as integers against the oracle's map.
template <int GRID, bool STORE_D, int NW, int CSTK, int COLS, bool STORE_K = false>
__global__ __launch_bounds__(64 * NW) void tile2_kernel(TileWalkArgs A, SsqParams sp) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int RPI = 64 / COLS, LGC = COLS == 32 ? 5 : 4;   // rows per wavefront instruction, log2 COLS
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & (COLS - 1), h = lane >> LGC, hb4 = (lane & ~(COLS - 1)) * 4;
    const int64_t N = A.N;
    const unsigned nN = (unsigned)N;
    const int na = (int)A.na, omax = na - 1;
    double2* T = reinterpret_cast<double2*>(lds_raw);          // (na + 1) x COLS cells, the last row: scratch
    for (int k = threadIdx.x; k < (na + 1) * COLS; k += 64 * NW) T[k] = make_double2(0.0, 0.0);
    __syncthreads();
    // (LDS byte addresses of the lane's column in row 0 and in the scratch row)
    const int c16 = c * 16 + (int)SSQ_LDS_ADDR(lds_raw);
    const int scratch16 = na * COLS * 16 + c16;
    const int full_rounds = na / (NW * RPI);                   // write-out rounds (NW * RPI rows each) that are complete

    // the walk over the tiles (ssq_tile_dev.h; SSQ_DEBUG_TILE2_CARRY=0 / SSQ_DEBUG_TILE2_XCD=0 in the launcher's
    // environment: no carry through the signals' boundaries / no XCD permutation); the tiles start at column 0
    constexpr int sh = 0;
    TILE_WALK_TILES(COLS, sh);
    const auto* waves = SSQ_CONST_PTR(int4, A.waves);
    const int i0 = waves[wv].x, i1 = waves[wv].y, isp = waves[wv].z, ni = i1 - i0;
    // The wavefronts of a SIMD compete for its issue slots and the oldest wins: left alone, the four
    // youngest wavefronts of the workgroup finish their rows of every tile last and the others wait
    // for them at the barrier (measured: 14.7 k of 37 k cycles per tile); fixed priorities against the
    // age only turn the order around. So the priorities rotate: the four wavefronts of a SIMD (w, w + 4,
    // w + 8, w + 12) alternate between two levels, two high and two low at any time, swapped with every
    // item (+2 %; four rotating levels measured the same and cost three more branches per item).
    int prio = (wv >> 2) & 1;
    auto rotate_priority = [&]() {
        SSQ_PRIO_TOGGLE(prio);                                 // (two levels, swapped with every item)
    };
    const float g2 = (float)(A.gamma * A.gamma);
    const float m2hi = g2 * 1.000004f, m2lo = g2 * 0.999996f;
    const int fx = sp.flipud ? -1 : 0, fa = sp.flipud ? na : 0;
    using TM = Term<float, CSTK == 2>;
    using w_t = typename TM::wtype;
    const auto* cstv = SSQ_CONST_PTR(w_t, A.cst);

    // ---- a tile's end: all terms in (barrier), every wavefront writes its share of the rows to
    // Tx and clears them, tile free again (barrier). A lane takes one cell -- column c of sub-row h -- per round: an
    // 8-byte store, a wavefront instruction = 64 / COLS rows, a round = NW * RPI rows of the workgroup. N even or
    // odd alike; a signal's partial last tile goes column by column under a mask.
    auto finish_tile = [&](int tx, int sg) {
        SSQ_WG_BARRIER();
        float2* Tx = A.Tx + (int64_t)(A.sig0 + sg) * na * N;
        constexpr int NA_CAP = COLS == 32 ? 320 : 512;
        {
            constexpr int ROUNDS = (NA_CAP + NW * RPI - 1) / (NW * RPI), RR = NW * RPI;    // RR rows per round
            const int k0 = wv * RPI + h;                       // the lane's row in round 0
            if ((tx + 1) * COLS <= (int)nN) {
                // every column of the tile exists (all but a signal's last tile when COLS does not divide N):
                // the rounds below the last need no masks -- scalar base per round + a per-lane constant
                char* tb = reinterpret_cast<char*>(Tx) + (size_t)tx * (COLS * 8);
                const unsigned voff = ((unsigned)k0 * nN + (unsigned)c) * 8u;
                // (the round count and the rounds' distance are re-read as scalars at every use: hoisted out
                // of the item loop, the compiler keeps ten lane masks and ten 64-bit offsets in spilled registers)
                int fr = full_rounds;
                size_t step = (size_t)RR * (size_t)N * 8;
#pragma unroll
                for (int m = 0; m < ROUNDS - 1; ++m) {
                    SSQ_OPAQUE_S(fr); SSQ_OPAQUE_S(step);
                    if (m < fr) {                              // (wave-uniform)
                        const int k = k0 + m * RR;
                        const double2 v = T[k * COLS + c];
                        T[k * COLS + c] = make_double2(0.0, 0.0);
                        *reinterpret_cast<float2*>(tb + (size_t)voff) = make_float2((float)v.x, (float)v.y);
                        tb += step;
                        asm volatile("" ::: "memory");         // (keeps the rounds from being batched into registers)
                    }
                }
                {   // the last round: the rows left, and the scratch row cleared by the lanes past them
                    const int k = k0 + fr * RR;
                    const int kc_ = k < na ? k : na;
                    const double2 v = T[kc_ * COLS + c];
                    T[kc_ * COLS + c] = make_double2(0.0, 0.0);
                    if (k < na)
                        *reinterpret_cast<float2*>(tb + (size_t)voff) = make_float2((float)v.x, (float)v.y);
                }
            } else {
                const unsigned col = (unsigned)(tx * COLS + c);
                const bool ok = col < nN;
#pragma unroll 1
                for (int m = 0; m * RR < na + 1; ++m) {
                    const int k = k0 + m * RR;
                    const int kc_ = k < na ? k : na;
                    const double2 v = T[kc_ * COLS + c];
                    T[kc_ * COLS + c] = make_double2(0.0, 0.0);
                    if (ok && k < na) Tx[(unsigned)k * nN + col] = make_float2((float)v.x, (float)v.y);
                }
            }
        }
        tile_count(A.counters);
        SSQ_WG_BARRIER();
    };

    if (ni <= 0) {                                             // more wavefronts than items: write-outs only
        TILE_WALK_FINISH_ONLY(finish_tile);
        return;
    }

    // ---- the wavefront's sequence of (tile, item) positions, software-pipelined over a ring of three
    // data slots (the loop is unrolled three times, the slots are compile-time): while position p is
    // computed, the data of p + 2 go out. Two cursors walk the same sequence (TILE_WALK_CURSORS), the
    // loads' two positions ahead of the arithmetic's. Past the last tile the loads' cursor stays on it (all
    // loads unconditional, see the note in tile_kernel: what they fetch there is valid and unused).
    TILE_WALK_CURSORS(COLS, A.n1);
    const int total = ntl * ni;                                // positions of this wavefront
    typedef int int8v __attribute__((ext_vector_type(8)));
    const auto* items = SSQ_CONST_PTR(int8v, A.items);
    // per-lane constants of the addresses: the lane's place inside an item's rows
    const unsigned lane_row8 = (unsigned)h * nN * 8u + (unsigned)c * 8u;       // bytes: sub-row h, column c
    const unsigned lane_col8 = (unsigned)c * 8u;

    // data of a position: (interpolated) the lane's sample of its sub-row's window, or (rows read
    // back) Wx and the bin of the lane's point
    struct Data { float2 u; int kq; };
    const char* const U8 = reinterpret_cast<const char*>(A.U);
    const char* const WX8 = reinterpret_cast<const char*>(A.Wx) + (size_t)((int64_t)A.sig0 * na * N) * 8u;
    const char* const KX8 = reinterpret_cast<const char*>(A.kidx);
    auto load_data = [&](const int8v R, const Pos& q) {
        Data d;
        const int w0 = R[0];
        const int kind = (w0 >> 12) & 1;
        const char* base; unsigned voff;
        const char* kbase = reinterpret_cast<const char*>(A.items); unsigned koff = (unsigned)lane * 2u;
        if (kind) {                                            // (wave-uniform; the loads themselves stay outside)
            // sample (qb + min(c, wlast)) mod L of row h of the item, h * L entries on
            const int lgR = (w0 >> 13) & 31;
            const int qb = (q.nabs0 >> lgR) - (TILE_W / 2 - 1);
            const int wlast = ((COLS - 1) >> lgR) + TILE_W;
            const int lmask = A.mmask >> lgR;                  // L - 1, L = M / R
            voff = (((unsigned)((qb + (c < wlast ? c : wlast)) & lmask)) + ((unsigned)h << (A.lgM - lgR))) * 8u;
            base = U8 + ((size_t)(unsigned)R[1] + (size_t)((unsigned)q.sg * (unsigned)R[3])) * 8u;
        } else {
            // point (row0 + h, column) -- the last column's for lanes past it, the last real row's for
            // padded sub-rows -- and its bin
            const int npad = (w0 >> 9) & 7;
            unsigned lr8 = lane_row8;
            if (RPI == 2) { if (npad) lr8 = lane_col8; }
            else if (npad) lr8 = (unsigned)min(h, RPI - 1 - npad) * nN * 8u + lane_col8;
            if (q.nabs0 == nabs_last) {                        // (the last tile may be partial)
                const int col = q.nabs0 - A.n1 + c;
                if (col >= (int)N) lr8 -= (unsigned)(col - ((int)N - 1)) * 8u;
            }
            voff = lr8;
            base = WX8 + ((size_t)q.off8 + (unsigned)R[2]);
            kbase = KX8 + (((size_t)q.off8 + (unsigned)R[2]) >> 2);
            koff = lr8 >> 2;
        }
        d.u = *reinterpret_cast<const float2*>(base + (size_t)voff);
        // (the bin: a load either way, from a harmless address for interpolated rows -- a conditional
        // load costs the compiler its count of loads in flight)
        d.kq = (int)*reinterpret_cast<const unsigned short*>(kbase + (size_t)koff);
        return d;
    };
    // the weights of the wavefront's (up to) two classes, for the lane's column phase: once
    ssq_f2 wta[TILE_W], wtb[TILE_W];
    auto load_wt = [&](ssq_f2 (&wt)[TILE_W], int it, int woff) {
        const int lgR = (items[it][0] >> 13) & 31;
        const int nabs = A.n1 + bid * COLS + c;                // (every tile of this workgroup: the same n mod R)
        const int R = 1 << lgR;
        const float4* wp = A.wtab + (int64_t)woff * 4 + (nabs & (R - 1));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 v = wp[t * R];
            wt[2 * t].x = v.x; wt[2 * t].y = v.y; wt[2 * t + 1].x = v.z; wt[2 * t + 1].y = v.w;
        }
    };
    load_wt(wta, i0, waves[wv].w & 0xFFFF);
    load_wt(wtb, isp < i1 ? isp : i0, (int)((unsigned)waves[wv].w >> 16));

    // (the loop below sits in a lambda called once, after the test `has0`, whose answer nothing reads: as they were
    // when a second, kind-free loop existed beside it. Inlined straight into the kernel, or without the test, the
    // same code compiles to other instructions -- other registers, or s_bitcmp0 for the kind test.)
    auto run = [&]() {
    Data D[3];
    Pos tc, tl;                                                // the tile of the arithmetic's cursor, of the loads'
    TILE_WALK_FIRST(tc, COLS, sh);
    tl = tc;
    if (total <= 0) return;
    int it_c = i0, it_l = i0;
    bool tc_last = tc.nabs0 == nabs_last && (N & (COLS - 1)) != 0;   // the arithmetic's tile is a signal's last, partial one
    int left = total;                                          // positions not yet finished
    auto step_loads = [&]() { if (++it_l >= i1) { it_l = i0; tl = next_tile(tl); } };
    // the records of the position in hand and of the one whose data go out next: asked for (through
    // the scalar cache) at the end of the position before, so that they are there when it starts
    int8v Rc = items[i0];
    D[0] = load_data(Rc, tl);
    step_loads();
    D[1] = load_data(items[it_l], tl);
    step_loads();
    // (the third slot: position 0 again -- a load like the loop's, so that the compiler's count of the loads in
    // flight at the loop's head is the loop's own; a plain copy made the first body wait for one load too many)
    D[2] = load_data(Rc, tc);
    int8v Rn = items[it_l];
    // the per-row reassignment weights of the position in hand (scalar loads, asked for with its records)
    w_t csn[RPI];
    auto load_cs = [&](int row0) {
        if (CSTK != 0) {
#pragma unroll
            for (int k = 0; k < RPI; ++k) csn[k] = cstv[min(row0 + k, omax)];
        }
    };
    load_cs(Rc[0] & 0x1FF);
    using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    bool more = true;
    auto body = [&](auto KK) {
        constexpr int k0 = decltype(KK)::value, k1 = (k0 + 1) % 3, k2 = (k0 + 2) % 3;
        const Pos pc = tc;
        rotate_priority();
        D[k2] = load_data(Rn, tl);                       // the data of p + 2
        step_loads();
        const Data dc = D[k0];
        const int w0 = Rc[0];
        const int npad = (w0 >> 9) & 7, kind = (w0 >> 12) & 1;
        const int nabs = pc.nabs0 + c;                         // (lanes past the last column: results unused)
        // (every lane's point counts, except in a class's last item -- padded sub-rows -- and in the last
        // tile of a signal when N is not a multiple of the tile: a wave-uniform test keeps the rest free)
        bool livept = true;
        if ((w0 & 0xE00) != 0 || tc_last) livept = h < RPI - npad && nabs - A.n1 < (int)N;
        int cell16; float tvx, tvy;
        if (kind == 0) {
            const int kk = dc.kq & 0xFFFF;
            cell16 = (livept && kk != TILE_NOBIN) ? kk * (COLS * 16) + c16 : scratch16;
            tvx = dc.u.x; tvy = dc.u.y;
            if constexpr (STORE_K) {
                char* kd8 = reinterpret_cast<char*>(A.kdump) + (((size_t)((int64_t)A.sig0 * na * N) * 8u + (size_t)pc.off8 + (unsigned)Rc[2]) >> 2);
                if (livept) *reinterpret_cast<unsigned short*>(kd8 + (size_t)(lane_row8 >> 2)) = (unsigned short)kk;
            }
        } else {
            const int lgR = (w0 >> 13) & 31;
            const int qb3 = pc.nabs0 >> lgR;                   // window start + 3: tap 0 of sample q0 sits in lane q0 - qb3
            const int baddr = (((nabs >> lgR) - qb3) << 2) + hb4;
            ssq_f2 A2, D2;
            {
                ssq_f2 sv[TILE_W];
                gather8(sv, baddr, dc.u.x, dc.u.y);
                // (A2 = (a_re, a_im), D2 = (a'_re, a'_im): the pairs the modulation multiplies)
                if (it_c < isp) {   // (wave-uniform: the wavefront's first or second class)
                    SSQ_TAPS8(A2, D2, wta, sv[0], sv[1], sv[2], sv[3], sv[4], sv[5], sv[6], sv[7]);
                } else {
                    SSQ_TAPS8(A2, D2, wtb, sv[0], sv[1], sv[2], sv[3], sv[4], sv[5], sv[6], sv[7]);
                }
            }
            int kcs = Rc[4];                                    // centre bin of the lane's row
#pragma unroll
            for (int k = 1; k < RPI; ++k) if (h == k) kcs = Rc[4 + k];
            const float theta = (float)kcs * A.theta_scale;
            // d/dt of e^{i theta n} a(n):  e^{i theta n} (i theta a + a')
            D2.x = __builtin_fmaf(-theta, A2.y, D2.x);
            D2.y = __builtin_fmaf(theta, A2.x, D2.y);
            const float rev = (float)(__umul24((unsigned)kcs, (unsigned)nabs) & (unsigned)A.mmask) * A.inv_m;
            ssq_f2 tw2, W2, V2;
            tw2.x = __builtin_amdgcn_cosf(rev); tw2.y = __builtin_amdgcn_sinf(rev);
            SSQ_CMUL_PK(W2, tw2, A2);
            SSQ_CMUL_PK(V2, tw2, D2);
            const float2 Wv = make_float2(W2.x, W2.y);
            const float2 Dv = make_float2(V2.x, V2.y);
            // (lanes past the last column hold another column's weights, padded sub-rows another row's
            // samples: their values go nowhere)
            char* wx8 = const_cast<char*>(WX8) + ((size_t)pc.off8 + (unsigned)Rc[2]);
            if (livept) *reinterpret_cast<float2*>(wx8 + (size_t)lane_row8) = Wv;
            if (STORE_D) {
                char* dwx8 = reinterpret_cast<char*>(A.dWx) + ((size_t)((int64_t)A.sig0 * na * N) * 8u + (size_t)pc.off8 + (unsigned)Rc[2]);
                if (livept) *reinterpret_cast<float2*>(dwx8 + (size_t)lane_row8) = Dv;
            }
            // phase transform and bin: as emit_point<LEAN> of the block kernels
            TILE_BIN_SCREEN(GRID, Wv, Dv);
            int kout = (above && livept) ? kf : -1;
            const bool pend = livept && !(below | (above & ok));
            if (pend) kout = exact_bin(Wv, Dv, sp, omax, A.gamma);
            cell16 = kout >= 0 ? kout * (COLS * 16) + c16 : scratch16;
            tvx = Wv.x; tvy = Wv.y;
            if constexpr (STORE_K) {
                char* kd8 = reinterpret_cast<char*>(A.kdump) + (((size_t)((int64_t)A.sig0 * na * N) * 8u + (size_t)pc.off8 + (unsigned)Rc[2]) >> 2);
                if (livept) *reinterpret_cast<unsigned short*>(kd8 + (size_t)(lane_row8 >> 2)) = (unsigned short)(kout >= 0 ? kout : TILE_NOBIN);
            }
        }
        {
            w_t cs = (w_t)A.cst0;
            if (CSTK != 0) {
                cs = csn[0];
#pragma unroll
                for (int k = 1; k < RPI; ++k) if (h == k) cs = csn[k];
            }
            const double ax = (double)TM::make(tvx, cs), ay = (double)TM::make(tvy, cs);
            SSQ_LDS_ADD_F64_AT(cell16, 0, ax);
            SSQ_LDS_ADD_F64_AT(cell16, 8, ay);
        }
        more = --left > 0;
        const bool tile_end = ++it_c >= i1;                    // (the block's last item: the tile is complete)
        if (tile_end) it_c = i0;
        Rc = items[it_c];                                      // the next position's records (see above)
        Rn = items[it_l];
        load_cs(Rc[0] & 0x1FF);                                // ... and its rows' weights, when there is one per row
        if (tile_end) {
            finish_tile((pc.nabs0 - A.n1) >> LGC, pc.sg);
            tc = next_tile(tc);
            tc_last = tc.nabs0 == nabs_last && (N & (COLS - 1)) != 0;
        }
    };
    for (;;) {
        body(K0{}); if (!more) break;
        body(K1{}); if (!more) break;
        body(K2{}); if (!more) break;
    }
    };
    // (does the block hold rows read back? It spans at most two classes: its first item and the first of its second
    // class tell. Measured: a second loop without the bin load and the kind tests for the wavefronts of interpolated
    // rows only -- one vector-memory instruction and ten scalar ones less per item -- is SLOWER, 230 vs 220 us)
    const bool has0 = !((items[i0][0] >> 12) & 1) || (isp < i1 && !((items[isp][0] >> 12) & 1));
    (void)has0;
    run();
}

// ---------------------------------------------------------------------------- host side
int TilePlan::run_f64(int sig, int nsig, float* Wx, float* dWx, float* Tx, const unsigned short* kidx,
                      const void* cst, float cst0, const SsqParams& sp, hipStream_t stream, unsigned short* kdump) {
    TileWalkArgs A = walk_args(items2, wave_first2, sig, nsig, Wx, dWx, Tx, kidx, cst, cst0, sp, kdump);
    // 16 wavefronts = one workgroup of 1024 work-items per CU (measured, round 4: 12 wavefronts 235 us against 220;
    // 16-column tiles with 16 wavefronts 245 us, with 8 wavefronts and two workgroups per CU 260-275 us --
    // profiles/r4_ab_history.txt); as many workgroups per CU as fit its LDS side by side, up to 2
    const size_t lds = tile2_lds_bytes(na, cols2);
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds, (size_t)(32 / TILE2_NW)));
    const int G = walk_grid((N + cols2 - 1) / cols2, cols2, per_cu, A);
    return tile_dispatch<2>(sp, dWx != nullptr, kdump != nullptr, [&](auto grid, auto d, auto cstk, auto k) {
        // (the bin dump beside a double per row: built for the 16-column tile, whose rows pass 256)
        if constexpr (k() && cstk() == 2) {
            SSQ_REQUIRE(cols2 == 16, "bin dump with float64 weights per row: built for the 16-column tile (na >= 320)");
        } else if (cols2 == 32)
            return tile_launch(tile2_kernel<grid(), d(), TILE2_NW, cstk(), 32, k()>, G, TILE2_NW, lds, A, sp, stream);
        return tile_launch(tile2_kernel<grid(), d(), TILE2_NW, cstk(), 16, k()>, G, TILE2_NW, lds, A, sp, stream);
    });
}

}  // namespace ssq
