// ssq_cwt_tiles.hip -- the column-tile path of the fused ssq_cwt form (float32, gfx950): the plan object.
//
// Math and planning: ssqueezepy_amd/_tiles.py. The device code lives in four translation units:
//   ssq_tile_fft.hip      the intermediates (decimated baseband samples of the interpolated rows; the analytic signal)
//   ssq_tile_pair.hip     tile3_kernel -- float64 Tx tile in LDS, unordered ds_add_f64, two columns per lane: the default
//   ssq_tile_f64.hip      tile2_kernel -- the same with one column per lane (16-column tiles for 320 .. 511 rows)
//   ssq_tile_ordered.hip  tile_kernel  -- float32 tile, terms added in the reference's row order by a ticket
//                         (SSQ_TILE_ORDER=ordered: Tx bit for bit the CPU loop's)
// (ssq_tile_dev.h: the device pieces they share.) Here: the tables the kernels walk (TilePlan::create), the choice
// between them (tile_kernel), the arguments and grid of tile2_kernel / tile3_kernel, what executed (tiles_done).
#include "ssq_common.h"
#include "ssq_tiles.h"
#include "ssq_ldsfft.h"
#include <algorithm>
#include <cmath>

namespace ssq {

int tile_rows_per_step() { return TILE_G; }

// The default kernels' items: `rpi` consecutive rows of a step, one record of 8 words per item:
// row0 | padded sub-rows << 9 | kind << 12 | lgR << 13 (| the weights' table offset << 18: tile3_kernel),
// samples of sub-row 0 (class offset + row in class * L), row0 * N * 8, entries between two signals' rows of the
// class, centre bins. tile2_kernel (ssq_tile_f64.hip): rpi = 64 / columns per tile; tile3_kernel
// (ssq_tile_pair.hip): 4 rows x 32 columns, two columns per lane.
struct ItemTable {
    int n = 0;
    std::vector<int32_t> rec;       // [n][8]
    std::vector<int32_t> cls;       // per item: 0 rows read back, 1 + lgR interpolated
    std::vector<int32_t> woff;      // per item: the weights' table offset (interpolated)
    bool ok = true;                 // the records can hold the tables (sub-rows consecutive, offsets in range)
};
static ItemTable pack_items(const TileSeg* sg, int nsegs, const TileRow* rw, int nsteps, int64_t M, int64_t N, int rpi,
                            bool woff_in_record) {
    ItemTable t;
    t.n = nsteps * TILE_G / rpi;
    t.rec.assign((size_t)t.n * 8, 0); t.cls.assign((size_t)t.n, 0); t.woff.assign((size_t)t.n, 0);
    for (int i = 0; i < nsegs; ++i) {
        const int64_t L = (int64_t)M >> sg[i].lgR;
        if (sg[i].kind && (sg[i].wtab_off >= (woff_in_record ? 16384 : 65536) || sg[i].sig_stride % L)) t.ok = false;
        for (int s = 0; s < sg[i].nsteps * TILE_G / rpi; ++s) {
            const size_t it = (size_t)sg[i].first * TILE_G / rpi + s;
            const TileRow* r = rw + it * rpi;
            int32_t* q = &t.rec[8 * it];
            int npad = 0;
            for (int k = 0; k < rpi; ++k) {
                if (r[k].row < 0) ++npad;
                else if (npad) t.ok = false;                      // padding trails
                // the sub-rows are consecutive rows of the class (the padding repeats the last one)
                if (r[k].row >= 0 && ((r[k].row & 0xFFFF) != (r[0].row & 0xFFFF) + k
                                      || (sg[i].kind && r[k].ubase != r[0].ubase + k * L))) t.ok = false;
                q[4 + k] = r[k].kc;
            }
            const int32_t row0 = r[0].row & 0xFFFF;
            q[0] = row0 | (npad << 9) | (sg[i].kind << 12) | (sg[i].lgR << 13)
                   | (woff_in_record && sg[i].kind ? (int32_t)((uint32_t)sg[i].wtab_off << 18) : 0);
            q[1] = sg[i].kind ? sg[i].cls_base + r[0].ubase : 0;
            q[2] = (int32_t)(uint32_t)((int64_t)row0 * N * 8);
            q[3] = sg[i].kind ? sg[i].sig_stride : 0;
            t.cls[it] = sg[i].kind ? 1 + sg[i].lgR : 0;
            t.woff[it] = sg[i].kind ? sg[i].wtab_off : 0;
        }
    }
    return t;
}

// tile2_kernel: contiguous, cost-balanced blocks of items per wavefront, each spanning at most TWO classes (kind /
// decimation): the kernel keeps the weights of (up to) two classes in registers. waves: [nw][4] = first item, end,
// first item of the second class, the weights' table offsets of the two classes (16 bits each). rb_cost: what an
// item of rows read back costs next to an interpolated one. Returns whether the kernel can take the items (t.ok, and
// they cut that way).
static bool cut_item_blocks(const ItemTable& t, int nw, float rb_cost, std::vector<int32_t>& waves) {
    const int n_items = t.n;
    bool ok = t.ok;
    std::vector<int> run_start;                        // maximal runs of one class
    for (int it = 0; it < n_items; ++it)
        if (it == 0 || t.cls[it] != t.cls[it - 1]) run_start.push_back(it);
    const int nruns = (int)run_start.size();
    run_start.push_back(n_items);
    std::vector<double> pre((size_t)n_items + 1, 0.0);
    for (int it = 0; it < n_items; ++it) pre[it + 1] = pre[it] + (t.cls[it] ? 1.0f : rb_cost);
    waves.clear();
    // (round 4 also sized the blocks by the wavefronts' measured speeds -- the older wavefronts of a SIMD finish the
    // same work 10-19 % sooner -- to no effect: 221 +- 3 us for every weighting; a SIMD's total is what counts)
    int cur = 0;
    const double stot = nw;
    double sacc = 0;
    for (int w = 0; w < nw; ++w) {
        sacc += 1.0;
        if (cur >= n_items) { waves.insert(waves.end(), {n_items, n_items, n_items, 0}); continue; }
        int r0 = 0;
        while (run_start[r0 + 1] <= cur) ++r0;
        const int maxe = run_start[std::min(r0 + 2, nruns)];          // at most the rest of this run and the next
        const int rem = nw - w - 1;
        const int rmin = std::max(r0, nruns - 2 * rem);               // the rest must fit the remaining wavefronts
        int mine = rem == 0 ? n_items : run_start[std::min(rmin, nruns)];
        mine = std::max(mine, cur + 1);
        int e = cur;
        const double want = pre[n_items] * sacc / stot;
        while (e < n_items && pre[e + 1] <= want + 1e-9) ++e;
        e = std::min(std::max(e, mine), maxe);
        if (rem == 0) { e = n_items; if (e > maxe) ok = false; }
        const int isp = run_start[r0 + 1] < e ? run_start[r0 + 1] : e;
        waves.insert(waves.end(), {cur, e, isp, t.woff[cur] | (t.woff[std::min(isp, n_items - 1)] << 16)});
        cur = e;
    }
    return ok && cur >= n_items;
}

// tile3_kernel: per-wavefront LISTS instead of contiguous row blocks. Round 6's stamps showed the wavefronts waiting
// 22 % of their time at the tile's end for the slowest of them (4-row items: a block is 4 or 5 items). So:
//   1. the interpolated items, class by class, are cut into `nw` chunks minimising the largest (a chunk of several
//      classes pays `chg_cost` items per class: the weights are re-read per tile);
//   2. the items of rows read back (`rb_cost` items each) need no weights: each goes to the wavefront with the least
//      work;
//   3. the item table is permuted so that a wavefront's list is contiguous (chunk, then rows read back).
// dealt: the permuted records; waves: [nw][4] = first item, end, first item of the list's second class (or of its
// rows read back, or its end), 0. Returns whether the kernel can take the items (t.ok -- else no list is dealt --
// and every item dealt).
static bool deal_item_lists(const ItemTable& t, int nw, float rb_cost, float chg_cost, std::vector<int32_t>& dealt,
                            std::vector<int32_t>& waves) {
    const int n_items = t.n;
    const std::vector<int32_t>& icls = t.cls;
    bool ok = t.ok;
    std::vector<int> iin, irb;
    for (int it = 0; it < n_items; ++it) (icls[it] ? iin : irb).push_back(it);
    const int ni = (int)iin.size();
    auto chunk_cost = [&](int a, int b) -> double {        // interpolated items [a, b) of `iin`
        if (b <= a) return 0.0;
        int ncl = 1;
        for (int j = a + 1; j < b; ++j) if (icls[iin[j]] != icls[iin[j - 1]]) ++ncl;
        return (double)(b - a) + (ncl > 1 ? chg_cost * ncl : 0.0);
    };
    // (the wavefronts of a SIMD do not run at one speed: the arbiter serves the oldest first, and the stamps show the
    // youngest taking a third longer per item. speed[w]: what wavefront w gets done relative to the mean, by its
    // age rank w / 4 -- chunk k goes to wavefront k, and "largest" above means largest time = cost / speed.)
    // (measured at config 2, one box: skew 0 / 0.1 / 0.2 / 0.3 -> 193-196 / 187 / 184-186 / 191 us with 16 wavefronts;
    // no gain with 12) -- four age ranks, skew 0.2: 1.2 .. 0.8
    static_assert(TILE3_NW == 16, "the speeds are those of four wavefronts per SIMD");
    std::vector<double> speed(nw);
    for (int w = 0; w < nw; ++w) speed[w] = 1.0 + 0.2f * (1.0 - 2.0 * (w / 4) / 3.0);
    std::vector<std::vector<double>> f(nw + 1, std::vector<double>(ni + 1, 1e30));
    std::vector<std::vector<int>> arg(nw + 1, std::vector<int>(ni + 1, 0));
    f[0][0] = 0.0;
    for (int k = 1; k <= nw; ++k)
        for (int j = 0; j <= ni; ++j)
            for (int a = 0; a <= j; ++a) {
                if (f[k - 1][a] >= 1e30) continue;
                const double c = std::max(f[k - 1][a], chunk_cost(a, j) / speed[k - 1]);
                // (ties: the later cut -- chunks of equal size rather than one long and one empty)
                if (c < f[k][j] - 1e-12 || (c <= f[k][j] + 1e-12 && a >= arg[k][j])) { f[k][j] = c; arg[k][j] = a; }
            }
    if (f[nw][ni] >= 1e30) ok = false;
    std::vector<std::vector<int>> lists(nw);
    std::vector<double> load(nw, 0.0);
    if (ok) {
        int j = ni;
        for (int k = nw; k >= 1; --k) {
            const int a = arg[k][j];
            for (int q = a; q < j; ++q) lists[k - 1].push_back(iin[q]);
            load[k - 1] = chunk_cost(a, j);
            j = a;
        }
        for (int it : irb) {
            int best = 0;
            for (int w = 1; w < nw; ++w)
                if ((load[w] + rb_cost) / speed[w] < (load[best] + rb_cost) / speed[best] - 1e-12) best = w;
            lists[best].push_back(it);
            load[best] += rb_cost;
        }
    }
    // (list k is wavefront k's: the speeds above are those of the wavefronts' slots)
    dealt.assign((size_t)n_items * 8, 0);
    waves.assign((size_t)nw * 4, 0);
    int pos = 0;
    for (int sl = 0; sl < nw; ++sl) {
        const std::vector<int>& L = lists[sl];
        const int first = pos;
        int isp = -1;
        for (size_t q = 0; q < L.size(); ++q) {
            if (q > 0 && icls[L[q]] && icls[L[q - 1]] && icls[L[q]] != icls[L[q - 1]] && isp < 0) isp = pos;
            memcpy(&dealt[(size_t)pos * 8], &t.rec[(size_t)L[q] * 8], 32);
            ++pos;
        }
        int e_int = first;
        for (size_t q = 0; q < L.size(); ++q) if (icls[L[q]]) e_int = first + (int)q + 1;
        if (isp < 0) isp = e_int;
        waves[4 * sl] = first; waves[4 * sl + 1] = pos; waves[4 * sl + 2] = isp;
    }
    return ok && pos == n_items;
}

int TilePlan::create(const ssq_cwt_tiles_desc& d, int64_t M_, int64_t N_, int64_t n1_, int64_t na_, int group_,
                     double dt_) {
    M = M_; N = N_; n1 = n1_; na = na_; group = group_; dt = dt_;
    nsegs = d.n_segs; nsteps = d.n_steps; n_irows = d.n_irows; u_total = d.u_total;
    SSQ_REQUIRE(nsegs >= 1 && nsteps >= 1 && n_irows >= 1 && d.n_classes >= 1, "empty tile tables");
    SSQ_REQUIRE((d.reserved ? d.reserved : 4) == TILE_G, "tile tables hold %d rows per step, this build walks %d",
                d.reserved ? d.reserved : 4, TILE_G);
    {
        int dev = 0; hipDeviceProp_t pr;
        SSQ_CHECK_HIP(hipGetDevice(&dev));
        SSQ_CHECK_HIP(hipGetDeviceProperties(&pr, dev));
        ncu = pr.multiProcessorCount;
        if (const char* e = getenv("SSQ_DEBUG_TILE_GRID")) if (atoi(e) > 0) ncu = atoi(e);
        // the tile kernels keep a tile of up to 160 KB in a workgroup's LDS (gfx950); a device with
        // less refuses the tile path here instead of failing at the first launch
        SSQ_REQUIRE((size_t)pr.maxSharedMemoryPerMultiProcessor >= 160 * 1024,
                    "the tile path needs 160 KB of LDS per workgroup, the device has %zu",
                    (size_t)pr.maxSharedMemoryPerMultiProcessor);
    }
    SSQ_REQUIRE(na * N < ((int64_t)1 << 29) && na < 512, "na = %lld, N = %lld: outside the tile path's 32-bit offsets",
                (long long)na, (long long)N);
    // the modulation phase kc * n mod M is formed with a 24-bit multiply and carried in a float
    // (and the centre bin, < M / 2, shares a word with the row: 22 bits)
    SSQ_REQUIRE(M <= ((int64_t)1 << 23), "the tile path needs a padded length <= 2^23");
    SSQ_REQUIRE((int64_t)group * u_total < ((int64_t)1 << 31), "tile intermediates exceed 2^31 entries");
    int rc;
    static_assert(sizeof(TileSeg) == 32 && sizeof(TileRow) == 16 && sizeof(TileIRow) == 32, "table layout");
    {   // one packed record per step (a wavefront's consecutive steps are usually of different
        // segments): kind | log2 R << 1 | weight-table offset << 8, L - 1, entries between two
        // signals' rows of the class, entries before the class
        std::vector<int32_t> hs((size_t)nsteps * 4);
        const TileSeg* sg = reinterpret_cast<const TileSeg*>(d.segs);
        int64_t covered = 0;
        for (int i = 0; i < nsegs; ++i) {
            SSQ_REQUIRE(sg[i].first == covered && sg[i].nsteps >= 1 && sg[i].first + sg[i].nsteps <= nsteps,
                        "tile segment %d does not continue the step list", i);
            SSQ_REQUIRE(sg[i].kind == 0 || sg[i].kind == 1, "tile segment %d: bad kind", i);
            SSQ_REQUIRE(sg[i].lgR >= 0 && sg[i].lgR < 32 && sg[i].wtab_off >= 0 && sg[i].wtab_off < (1 << 23),
                        "tile segment %d does not fit its packed record", i);
            for (int t = 0; t < sg[i].nsteps; ++t) {
                int32_t* q = &hs[((size_t)sg[i].first + t) * 4];
                q[0] = sg[i].kind | (sg[i].lgR << 1) | (sg[i].wtab_off << 8);
                q[1] = sg[i].lmask; q[2] = sg[i].sig_stride; q[3] = sg[i].cls_base;
            }
            covered += sg[i].nsteps;
        }
        SSQ_REQUIRE(covered == nsteps, "tile segments cover %lld of %d steps", (long long)covered, nsteps);
        if ((rc = mem.upload(&steps, hs.data(), hs.size() * 4))) return rc;
    }
    {   // row records as the kernel reads them: row | padding << 9 | centre bin << 10, offset of the
        // row's samples inside its class
        const TileRow* rw = reinterpret_cast<const TileRow*>(d.rows);
        std::vector<int32_t> hp((size_t)nsteps * TILE_G * 2);
        for (size_t i = 0; i < (size_t)nsteps * TILE_G; ++i) {
            const int32_t row = rw[i].row & 0xFFFF;
            SSQ_REQUIRE(row < 512 && rw[i].kc >= 0 && rw[i].kc < (1 << 22), "tile row %zu does not fit its packed record", i);
            hp[2 * i] = row | (rw[i].row < 0 ? 0x200 : 0) | (int32_t)((uint32_t)rw[i].kc << 10);
            hp[2 * i + 1] = rw[i].ubase;
        }
        if ((rc = mem.upload(&rows, hp.data(), hp.size() * 4))) return rc;
    }
    {   // the default kernels' items (see pack_items) and the wavefronts' shares of them
        const TileRow* rw = reinterpret_cast<const TileRow*>(d.rows);
        const TileSeg* sg = reinterpret_cast<const TileSeg*>(d.segs);
        cols2 = tile2_lds_bytes(na, 32) <= 160 * 1024 ? 32 : 16;
        SSQ_REQUIRE(tile2_lds_bytes(na, cols2) <= 160 * 1024, "na = %lld: the Tx tile exceeds the LDS", (long long)na);
        lgr_max2 = 0;
        for (int i = 0; i < nsegs; ++i) if (sg[i].kind) lgr_max2 = std::max(lgr_max2, (int)sg[i].lgR);
        std::vector<int32_t> waves;
        // tile2_kernel: rpi = 64 / columns per tile. (What a row read back costs next to an interpolated one when the
        // rows are dealt to the wavefronts; measured 0.5 .. 1.2: 221 / 223 / 222 / 228 / 225 us, round 4)
        ItemTable t2 = pack_items(sg, nsegs, rw, nsteps, M, N, 64 / cols2, false);
        tile2_ok = cut_item_blocks(t2, TILE2_NW, 0.7f, waves);
        n_items2 = t2.n;
        if ((rc = mem.upload(&items2, t2.rec.data(), t2.rec.size() * 4))) return rc;
        if ((rc = mem.upload(&wave_first2, waves.data(), waves.size() * 4))) return rc;
        tile3_ok = false;
        if (cols2 == 32) {
            // tile3_kernel: 4 rows x 32 columns, two columns per lane. (Measured with shader-clock stamps, round 6: an
            // item of rows read back costs 0.45 of an interpolated one, re-reading a class's weights 0.65)
            ItemTable t3 = pack_items(sg, nsegs, rw, nsteps, M, N, 4, true);
            std::vector<int32_t> dealt;
            tile3_ok = deal_item_lists(t3, TILE3_NW, 0.45f, 0.65f, dealt, waves);
            n_items3 = t3.n;
            if ((rc = mem.upload(&items3, dealt.data(), dealt.size() * 4))) return rc;
            if ((rc = mem.upload(&wave_first3, waves.data(), waves.size() * 4))) return rc;
            // (the 16 lanes of a sub-row hold the sample window of the tile's 32 columns: (31 >> lgR) + 8 + 1 <= 16 needs
            // a decimation of 4 or more -- R_MIN of _tiles.py; plans with a smaller one go to tile2_kernel)
            for (int i = 0; i < nsegs; ++i) if (sg[i].kind && sg[i].lgR < 2) tile3_ok = false;
        }
    }
    {   // weights, per class (R phases from wtab_off on): [phase][4 tap pairs] -> [tap pair][phase]
        const TileSeg* sg = reinterpret_cast<const TileSeg*>(d.segs);
        const float* src = reinterpret_cast<const float*>(d.wtab);
        std::vector<float> w((size_t)16 * d.n_phases, 0.f);
        std::vector<char> done((size_t)d.n_phases, 0);
        for (int i = 0; i < nsegs; ++i) {
            if (sg[i].kind != 1) continue;
            const int64_t R = (int64_t)1 << sg[i].lgR, o = sg[i].wtab_off;
            SSQ_REQUIRE(o >= 0 && o + R <= d.n_phases, "tile segment %d: weights outside the table", i);
            if (done[(size_t)o]) continue;
            done[(size_t)o] = 1;
            for (int64_t ph = 0; ph < R; ++ph)
                for (int t = 0; t < 4; ++t)
                    for (int k = 0; k < 4; ++k)
                        w[(size_t)(16 * o + (t * R + ph) * 4 + k)] = src[(size_t)(16 * (o + ph) + 4 * t + k)];
        }
        if ((rc = mem.upload(&wtab, w.data(), (size_t)64 * d.n_phases))) return rc;
    }
    if ((rc = mem.upload(&tbank, d.tbank, (size_t)4 * d.n_tbank))) return rc;
    cls.resize(d.n_classes);
    // classes of 2^14 entries and more: four-step kernels, L = A B with A <= B, both 128 .. 2048
    // (SSQ_DEBUG_TILE_FFT=rocfft keeps every class on rocFFT)
    const bool own_fft = !env_equals("SSQ_DEBUG_TILE_FFT", "rocfft");
    int64_t y_entries = 0;
    for (int c = 0; c < d.n_classes; ++c) {
        cls[c] = {d.classes[4 * c], d.classes[4 * c + 1], d.classes[4 * c + 2], 0, 0, 0};
        SSQ_REQUIRE(cls[c].L >= 2 && (cls[c].L & (cls[c].L - 1)) == 0 && cls[c].nrows >= 1, "bad tile class %d", c);
        lmax = std::max(lmax, cls[c].L);
        int lg = 0;
        while (((int64_t)1 << lg) < cls[c].L) ++lg;
        if (own_fft && lg >= 13 && lg <= 22) {
            cls[c].B = 1 << ((lg + 1) / 2); cls[c].A = 1 << (lg / 2);
            y_entries += (int64_t)group * cls[c].nrows * cls[c].L;
        } else if (own_fft && lg >= 6 && lg <= 12) {
            cls[c].B = 1;                              // one-pass kernel
        }
    }
    std::vector<TileIRow> hi;
    hi.reserve((size_t)n_irows);
    for (int pass = 0; pass < 2; ++pass)            // rows sorted by class, the four-step classes first
        for (int c = 0; c < d.n_classes; ++c) {
            if ((cls[c].A > 0 || cls[c].B > 0) != (pass == 0)) continue;
            if (pass == 1 && n_irows_fft == 0) first_irow_fft = (int)hi.size();
            cls[c].first = (int)hi.size();
            for (int r = 0; r < n_irows; ++r) {
                const int64_t* q = d.irows + 8 * r;
                if ((int)q[6] != c) continue;
                SSQ_REQUIRE(q[4] == cls[c].L && q[2] >= 1 && 2 * q[2] <= q[4]
                            && q[1] >= 0 && q[1] + q[2] <= M / 2 + 1 && q[5] >= 0 && q[5] + q[2] <= d.n_tbank
                            && q[7] >= 0 && q[7] < cls[c].nrows, "bad tile row %d", r);
                hi.push_back({(int32_t)q[0], (int32_t)q[1], (int32_t)q[2], (int32_t)q[3], (int32_t)q[4], (int32_t)q[5],
                              (int32_t)((int64_t)group * cls[c].upre + q[7] * cls[c].L), (int32_t)(cls[c].nrows * cls[c].L)});
            }
            SSQ_REQUIRE((int64_t)hi.size() - cls[c].first == cls[c].nrows, "tile class %d: %lld rows listed, %lld declared",
                        c, (long long)((int64_t)hi.size() - cls[c].first), (long long)cls[c].nrows);
            if (pass == 1) n_irows_fft += (int)cls[c].nrows;
        }
    SSQ_REQUIRE((int)hi.size() == n_irows, "tile rows of unknown classes");
    if ((rc = mem.upload(&irows, hi.data(), sizeof(TileIRow) * n_irows))) return rc;
    if (own_fft) {
        if ((rc = mem.alloc(&Y, (size_t)8 * y_entries))) return rc;
        std::vector<float> tw;
        for (int s = 0; s < 7; ++s) {
            const int Lp = 64 << s;
            ftw_off[s] = (int64_t)tw.size() / 2;
            fft_twiddles(Lp, tw);
        }
        if ((rc = mem.upload(&ftw, tw.data(), tw.size() * 4))) return rc;
    }
    // (+ 4 rows of slack: tile2_kernel's padded sub-rows read, and discard, the rows behind a class's last)
    if ((rc = mem.alloc(&U, (size_t)8 * (group * u_total + 4 * lmax)))) return rc;
    SSQ_CHECK_HIP(hipMemset(U, 0, (size_t)8 * (group * u_total + 4 * lmax)));
    if ((rc = mem.alloc(&counters, 4096))) return rc;        // [0]: tiles done
    SSQ_CHECK_HIP(hipMemset(counters, 0, 4096));
    for (size_t c = 0; c < cls.size(); ++c) {
        FftPlan fp;
        if (!cls[c].A && !cls[c].B) {
            rc = fp.create(1, SSQ_F32, (size_t)cls[c].L, (size_t)(group * cls[c].nrows), 1.0);
            if (rc) { fp.destroy(); return rc; }
        }
        ffts.push_back(fp);
    }
    for (int t = 0; t < 5; ++t) n_items_tile[t] = d.n_items_tile[t];
    SSQ_CHECK_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    SSQ_CHECK_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    SSQ_CHECK_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    return 0;
}

void TilePlan::destroy() {
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); side = nullptr; }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    ev_fork = ev_join = nullptr;
    for (auto& f : ffts) f.destroy();
    ffts.clear();
    mem.release();
}

int64_t TilePlan::bytes() const {
    int64_t b = mem.bytes();
    for (const FftPlan& f : ffts) b += (int64_t)f.work_bytes;
    return b;
}

// SSQ_TILE_ORDER = ordered: the ticketed kernel (float32 sums in the reference's order, bit for bit; na <=
// 318: tile_lds_bytes); default: tile3_kernel, or tile2_kernel (float64 tile, unordered adds: the same bins, sums
// rounded once; 32 columns for na <= 319, 16 columns for 320 .. 511: tile2_lds_bytes)
bool tile_ordered() { return reassign_ordered(); }
int TilePlan::tile_kernel() const {
    const int ordered = tile_lds_bytes(na) <= 160 * 1024 ? 1 : 0;    // (its 64-column float32 tile fits the LDS)
    if (tile_ordered()) return ordered;
    // tile3_kernel (two columns per lane): 32-column tiles (up to 319 rows); SSQ_DEBUG_TILE_PAIR=0 keeps tile2_kernel
    const char* e = getenv("SSQ_DEBUG_TILE_PAIR");
    if (tile3_ok && cols2 == 32 && N >= 64 && !(e && atoi(e) == 0)) return 3;
    return tile2_ok ? 2 : ordered;
}
int TilePlan::tile_cols() const {
    switch (tile_kernel()) {
    case 1: return TILE_COLS;
    case 2: return cols2;
    case 3: return 32;
    default: return 0;
    }
}

int TilePlan::run(int sig, int nsig, float* Wx, float* dWx, float* Tx, const unsigned short* kidx,
                  const void* cst, float cst0, const SsqParams& sp, hipStream_t stream, unsigned short* kdump) {
    switch (tile_kernel()) {
    case 3: return run_pair(sig, nsig, Wx, dWx, Tx, kidx, cst, cst0, sp, stream, kdump);
    case 2: return run_f64(sig, nsig, Wx, dWx, Tx, kidx, cst, cst0, sp, stream, kdump);
    case 1:
        SSQ_REQUIRE(!kdump, "bin dump: the default tile kernels only (unset SSQ_TILE_ORDER)");
        return run_ordered(sig, nsig, Wx, dWx, Tx, kidx, cst, cst0, sp, stream);
    default:
        set_error("na = %lld: no tile kernel can run in this mode (the executor asks usable() first)", (long long)na);
        return -1;
    }
}

TileWalkArgs TilePlan::walk_args(const void* items, const int32_t* waves, int sig, int nsig, float* Wx, float* dWx,
                                 float* Tx, const unsigned short* kidx, const void* cst, float cst0,
                                 const SsqParams& sp, unsigned short* kdump) const {
    TileWalkArgs A{};
    A.items = reinterpret_cast<const int*>(items); A.waves = reinterpret_cast<const int4*>(waves);
    A.wtab = (const float4*)wtab; A.U = (const float2*)U; A.cst = cst;
    A.Wx = (float2*)Wx; A.dWx = (float2*)dWx; A.Tx = (float2*)Tx; A.kidx = kidx; A.kdump = kdump;
    A.N = N; A.na = na; A.n1 = (int)n1; A.mmask = (int)(M - 1);
    A.lgM = 0; while (((int64_t)1 << A.lgM) < M) ++A.lgM;
    A.sig0 = sig; A.nsig = nsig; A.carry = 0; A.xcd = 0;
    A.inv_m = 1.0f / (float)M; A.theta_scale = (float)(6.283185307179586 / ((double)M * dt)); A.cst0 = cst0;
    A.counters = counters; A.gamma = sp.gamma;
    return A;
}

int TilePlan::walk_grid(int64_t ntx, int cols, int per_cu, TileWalkArgs& A) const {
    // Persistent workgroups, workgroup b walks tiles b, b + G, ... of every signal. The kernels keep a lane's
    // interpolation weights for the whole launch, so the columns of a workgroup's tiles must agree mod R for every
    // class: G * cols a multiple of the largest R (or a single tile per signal and workgroup).
    const int64_t cap = (int64_t)ncu * per_cu;
    const int64_t q = std::max<int64_t>(1, ((int64_t)1 << lgr_max2) / cols);
    const int64_t G = ntx <= cap ? ntx : std::max<int64_t>(q, cap / q * q);
    // ... and through the signals' boundaries when a signal's tile count keeps that phase too
    // (SSQ_DEBUG_TILE2_CARRY=0: every signal's walk starts at the workgroup's own tile)
    const char* ce = getenv("SSQ_DEBUG_TILE2_CARRY");
    A.carry = (!(ce && atoi(ce) == 0) && ntx > G && ntx % q == 0) ? 1 : 0;
    const char* xe = getenv("SSQ_DEBUG_TILE2_XCD");
    A.xcd = !(xe && atoi(xe) == 0) && G >= 16;
    return (int)G;
}

int64_t TilePlan::tiles_done(hipStream_t stream) {
    unsigned long long v = 0;
    if (!counters) return 0;
    if (hipStreamSynchronize(stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, counters, 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

}  // namespace ssq
