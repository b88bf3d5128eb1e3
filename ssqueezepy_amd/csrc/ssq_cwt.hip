// ssq_cwt.hip -- CWT / synchrosqueezed-CWT plan (C ABI: ssq_cwt_*): creation, the tables of the
// fast paths, and the orchestration of one execute.
//
// Per launch group of signals (reference: ssqueezepy/_cwt.py:255-306, _ssq_cwt.py:250-289):
//   x (N) --pad_kernel--> xp (M) --rocFFT R2C--> xh (M/2+1)                       (whole batch)
//   fast paths, when the plan has them (padded power-of-two length, analytic bank):
//     block rows   ssq_cwt_blocks.hip: blockzoom kernels (overlap-save blocks, LDS FFTs) ->
//                  Wx (+ dWx / w / 2-byte bin map)
//     exact rows   ssq_cwt_blocks.hip: four-step full-length FFT for the rows whose band is cut
//                  by the Nyquist bin (float32)
//     tile rows    ssq_cwt_tiles.hip (fused ssq_cwt form only): decimated baseband samples on a
//                  side stream, then the column-tile kernel: Wx of the interpolated rows and Tx
//                  of ALL rows (reads back the Wx + bins the block / exact kernels left)
//   generic path (any length / padtype None / rpadded / non-analytic banks), in row chunks:
//     xh, banded bank --bank_multiply_kernel--> P = psih*xh, dP = P*(1j*xi/dt)
//     --rocFFT C2C inverse, batched, scaled 1/M, in place--> padded Wx, dWx
//     --cwt_epilogue_kernel--> Wx[:, n1:n1+N] (+ dWx / w / bin map)
//   without the tile path: bin map or w --accumulate kernels (ssq_kernels.hip)--> Tx
// The backward pass (ssq_cwt_adjoint: gWx, gdWx -> gx) is at the end of the file.
// Only the returned arrays (Wx, Tx [, dWx, w]) are written at full size; padded intermediates
// live in plan-owned workspaces reused chunk after chunk.
//
// The bank is *banded*: each row keeps only the contiguous run of DFT bins on which the wavelet
// is non-negligible (7 % of na*M at N=160k), so it stays in the 256 MiB Infinity Cache across calls.
//
// Compiled with -ffp-contract=off (the epilogue computes bin indices; see ssq_kernels.hip).
#include "ssq_common.h"
#include "ssq_fft.h"
#include "ssq_blocks.h"
#include "ssq_tiles.h"
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace ssq {

// from ssq_kernels.hip (same arithmetic, re-declared here as device inlines would
// need a shared header; kept in one place via this include)
#include "ssq_point_math.inl"

template <typename T>
__global__ __launch_bounds__(256) void bank_multiply_kernel(
    const T* __restrict__ xh,        // (M/2+1) complex, spectrum of the real padded signal
    const T* __restrict__ bank, const int64_t* __restrict__ band_off,
    const int32_t* __restrict__ band_lo,
    T* __restrict__ prod,            // [rows][nplanes][M] complex
    int64_t M, const int32_t* __restrict__ rowlist, int64_t row0, int nplanes, double h, T inv_dt) {
    const int64_t r = blockIdx.y;            // row within the chunk
    const int64_t i = rowlist[row0 + r];
    const int64_t lo = band_lo[i];
    const int64_t off = band_off[i];
    const int64_t len = band_off[i + 1] - off;
    T* P = prod + (size_t)r * nplanes * 2 * M;
    T* dP = P + 2 * M;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < M;
         k += (int64_t)gridDim.x * blockDim.x) {
        T re = T(0), im = T(0), dre = T(0), dim = T(0);
        int64_t t = k - lo;
        if (t >= 0 && t < len) {
            T psi = bank[off + t];
            T a, b;
            if (k <= M / 2) { a = xh[2 * k]; b = xh[2 * k + 1]; }
            else { a = xh[2 * (M - k)]; b = -xh[2 * (M - k) + 1]; }
            re = psi * a; im = psi * b;
            if (nplanes > 1) {
                // xi_k = k*h (k <= M/2) or (k-M)*h, formed in double and stored in T
                // (wavelets.py:473-484); multiplier 1j*xi/dt as NumPy forms it: xi * (1/dt)
                int64_t ks = k <= M / 2 ? k : k - M;
                T m = (T)((double)ks * h) * inv_dt;
                dre = -(im * m); dim = re * m;
            }
        }
        P[2 * k] = re; P[2 * k + 1] = im;
        if (nplanes > 1) { dP[2 * k] = dre; dP[2 * k + 1] = dim; }
    }
}

struct EpilogueArgs {
    void* Wx; void* dWx; void* w; unsigned short* kidx;
    int64_t out_cols;     // N, or M when rpadded
    int64_t col0;         // n1, or 0 when rpadded
    int64_t row0;
    const int32_t* rowlist;
    const void* row_scale;
    double gamma;
    int have_ssq;
};

template <typename T>
__global__ __launch_bounds__(256) void cwt_epilogue_kernel(const T* __restrict__ prod, int64_t M,
                                                           int nplanes, int64_t na,
                                                           EpilogueArgs ea, SsqParams sp) {
    const int64_t r = blockIdx.y;
    const int64_t i = ea.rowlist[ea.row0 + r];
    const T* P = prod + (size_t)r * nplanes * 2 * M;
    const T* dP = P + 2 * M;
    const int64_t omax = na - 1;
    T rs = ea.row_scale ? ((const T*)ea.row_scale)[i] : T(1);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ea.out_cols;
         j += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = ea.col0 + j;
        int64_t q = i * ea.out_cols + j;
        T c = P[2 * p], d = P[2 * p + 1];
        if (ea.row_scale) { c = c * rs; d = d * rs; }
        ((T*)ea.Wx)[2 * q] = c; ((T*)ea.Wx)[2 * q + 1] = d;
        if (nplanes > 1) {
            T a = dP[2 * p], b = dP[2 * p + 1];
            if (ea.row_scale) { a = a * rs; b = b * rs; }
            if (ea.dWx) { ((T*)ea.dWx)[2 * q] = a; ((T*)ea.dWx)[2 * q + 1] = b; }
            if (ea.w) {
                // two-step form: phase_cwt (algos.py:720-740), threshold |Wx| < gamma
                T wv;
                if (mag_lt(c, d, (T)ea.gamma)) wv = (T)INFINITY;
                else wv = (T)fabs(phase_ratio(a, b, c, d));
                ((T*)ea.w)[q] = wv;
            }
            if (ea.kidx) {
                // fused form (algos.py:859-953), threshold |Wx| > gamma
                unsigned short kk = 0xFFFFu;
                if (mag_gt(c, d, ea.gamma)) {
                    int64_t k = bin_of_point(a, b, c, d, false, T(0), sp, omax);
                    kk = (unsigned short)(sp.flipud ? omax - k : k);
                }
                ea.kidx[kidx_index(i, j, na, ea.out_cols)] = kk;
            }
        }
    }
}

}  // namespace ssq

using namespace ssq;

// Optional per-stage HIP-event timing of an execute (ssq_cwt_plan_timing; bench.py --full reads it): 0 = pad + forward
// FFT + block spectra + the tile path's decimated samples, 1 = block rows, 2 = exact / generic rows, 3 = reassignment.
// Two events bracket the front of an execute, six belong to each launch group: the four boundaries of its stages 1 - 3
// and the pair around its decimated samples.
struct StageTimer {
    enum Mark { ROWS = 0, OTHER_ROWS = 1, REASSIGN = 2, GROUP_END = 3, SAMPLES = 4, SAMPLES_END = 5 };
    bool enabled = false;                 // what ssq_cwt_plan_timing asked for
    bool on = false;                      // this execute is timed
    std::vector<hipEvent_t> tev;
    hipStream_t stream = nullptr;
    double stage_ms[4] = {0, 0, 0, 0};
    int64_t signals = 0;
    int begin(int64_t groups, hipStream_t s) {
        on = enabled; stream = s;
        while (on && tev.size() < (size_t)(2 + 6 * groups)) {
            hipEvent_t e; SSQ_CHECK_HIP(hipEventCreate(&e)); tev.push_back(e);
        }
        if (on) (void)hipEventRecord(tev[0], stream);
        return 0;
    }
    void front_done() { if (on) (void)hipEventRecord(tev[1], stream); }
    void mark(int64_t group, Mark m) { if (on) (void)hipEventRecord(tev[(size_t)(2 + 6 * group + m)], stream); }
    // waits for the last group and adds the execute's stages up
    int finish(int64_t groups, bool samples, int64_t batch) {
        if (!on) return 0;
        SSQ_CHECK_HIP(hipEventSynchronize(tev[(size_t)(2 + 6 * (groups - 1) + GROUP_END)]));
        auto add = [&](int stage, size_t from, size_t to) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, tev[from], tev[to]); stage_ms[stage] += ms;
        };
        add(0, 0, 1);
        for (int64_t g = 0; samples && g < groups; ++g) add(0, (size_t)(2 + 6 * g + SAMPLES), (size_t)(2 + 6 * g + SAMPLES_END));
        for (int64_t g = 0; g < groups; ++g)
            for (int st = 0; st < 3; ++st) add(1 + st, (size_t)(2 + 6 * g + st), (size_t)(2 + 6 * g + st + 1));
        signals += batch;
        return 0;
    }
    void reset(bool enable) { enabled = enable; for (double& v : stage_ms) v = 0; signals = 0; }
    void destroy() { for (hipEvent_t e : tev) (void)hipEventDestroy(e); tev.clear(); }
};

struct ssq_cwt_plan {
    ssq_cwt_desc d;
    int csize() const { return d.dtype == SSQ_F32 ? 8 : 16; }
    int rsize() const { return d.dtype == SSQ_F32 ? 4 : 8; }
    DeviceArena mem;                      // every device pointer below, the lazily made ones too
    // device copies
    void* bank = nullptr; int64_t* band_off = nullptr; int32_t* band_lo = nullptr;
    void* row_scale = nullptr;
    std::vector<int64_t> h_band_off; std::vector<int32_t> h_band_lo;
    // workspace
    void* xp = nullptr; void* xh = nullptr; void* prod = nullptr; unsigned short* kidx = nullptr;
    int64_t rows_chunk = 0;
    size_t prod_bytes = 0;                // size of `prod` once it is allocated
    // signals per launch group: the fast-path kernels and the reassignment take `group`
    // signals as a grid dimension (fewer, longer launches; the bin map holds `group` maps)
    int group = 1;
    FftPlan fwd;                          // R2C, batch = max_batch
    std::map<int64_t, FftPlan> inv;       // C2C inverse keyed by transform count
    // ssq
    bool have_ssq = false; SsqParams sp{}; void* cst = nullptr;   // cst: the current entry of `weights`
    WeightVersions weights;
    float cst0 = 0.f;                     // first weight (all of them when sp.cst_uniform)
    PlanOrder order;
    std::string algo = "rocfft";
    // rows evaluated by the exact full-length path (all rows unless a block plan
    // took some over)
    int32_t* gen_rows = nullptr; int64_t n_gen = 0;
    int32_t* all_rows = nullptr;          // identity list (rpadded output bypasses blocks)
    const int32_t* gen_rows_for(bool use_blocks) const { return use_blocks ? gen_rows : all_rows; }
    BlockPlan* blk = nullptr;
    TilePlan* tile = nullptr;             // column-tile path of the fused ssq form (ssq_cwt_tiles.hip)
    bool executed = false;
    unsigned short* kdump = nullptr;      // diagnostic (ssq_cwt_plan_set_bin_dump): caller-owned (batch, na, n) bin map
    // the adjoint (ssq_cwt_adjoint), built at its first call: the spectrum sums (max_batch, m) complex, the inverse
    // pad map, the rows that reach each segment of ADJ_SEG bins, and the row transforms keyed by their count
    void* adj_spec = nullptr;
    int32_t* adj_off = nullptr; int32_t* adj_idx = nullptr; int32_t* adj_seg = nullptr;
    std::map<int64_t, FftPlan> adj_fwd;
    StageTimer timer;
    // device memory of the plan and of everything it owns (ssq_cwt_plan_bytes)
    int64_t bytes() const {
        int64_t b = mem.bytes() + (int64_t)fwd.work_bytes + (blk ? blk->bytes() : 0) + (tile ? tile->bytes() : 0);
        for (auto& kv : inv) b += (int64_t)kv.second.work_bytes;
        for (auto& kv : adj_fwd) b += (int64_t)kv.second.work_bytes;
        return b;
    }
};

static void destroy_blocks(BlockPlan* b) { b->destroy(); delete b; }
static void destroy_tiles(TilePlan* t) { t->destroy(); delete t; }

// the plan's transform of `count` rows in `plans`, made at its first use, over `data` in place
static int cwt_cached_fft(ssq_cwt_plan* pl, std::map<int64_t, FftPlan>& plans, int kind, int64_t count, double scale,
                          void* data, hipStream_t stream) {
    auto it = plans.find(count);
    if (it == plans.end()) {
        FftPlan fp;
        int rc = fp.create(kind, pl->d.dtype, (size_t)pl->d.m, (size_t)count, scale);
        if (rc) { fp.destroy(); return rc; }
        it = plans.emplace(count, fp).first;
    }
    return it->second.execute(data, nullptr, stream);
}
// the product workspace of the generic route and of the adjoint, made by the first call that needs it
static int cwt_product_workspace(ssq_cwt_plan* pl) { return pl->prod ? 0 : pl->mem.alloc(&pl->prod, pl->prod_bytes); }

extern "C" {

int ssq_cwt_plan_create(ssq_cwt_plan** out, const ssq_cwt_desc* desc) {
    SSQ_REQUIRE(out && desc, "ssq_cwt_plan_create: null pointer");
    const ssq_cwt_desc& d = *desc;
    SSQ_REQUIRE(d.dtype == SSQ_F32 || d.dtype == SSQ_F64, "bad dtype %d", d.dtype);
    SSQ_REQUIRE(d.n >= 1 && d.m >= d.n && d.na >= 1, "bad sizes n=%lld m=%lld na=%lld",
                (long long)d.n, (long long)d.m, (long long)d.na);
    SSQ_REQUIRE(d.n1 >= 0 && d.n1 + d.n <= d.m, "bad left pad %lld", (long long)d.n1);
    SSQ_REQUIRE(d.padtype >= SSQ_PAD_NONE && d.padtype <= SSQ_PAD_WRAP, "bad padtype %d", d.padtype);
    SSQ_REQUIRE(d.padtype != SSQ_PAD_NONE || d.m == d.n, "padtype NONE requires m == n");
    SSQ_REQUIRE(d.bank && d.band_off && d.band_lo, "bank arrays must not be null");
    SSQ_REQUIRE(d.dt > 0, "dt must be > 0");
    SSQ_REQUIRE(d.na < 65535, "na must be < 65535");
    for (int64_t i = 0; i < d.na; ++i) {
        int64_t len = d.band_off[i + 1] - d.band_off[i];
        SSQ_REQUIRE(len >= 0 && d.band_lo[i] >= 0 && d.band_lo[i] + len <= d.m,
                    "row %lld: band [%d, +%lld) outside [0, %lld)", (long long)i, d.band_lo[i],
                    (long long)len, (long long)d.m);
    }
    PlanGuard<ssq_cwt_plan> pl(new ssq_cwt_plan(), ssq_cwt_plan_destroy);
    pl->d = d;
    if (pl->d.max_batch < 1) pl->d.max_batch = 1;
    pl->h_band_off.assign(d.band_off, d.band_off + d.na + 1);
    pl->h_band_lo.assign(d.band_lo, d.band_lo + d.na);
    pl->d.bank = nullptr; pl->d.band_off = nullptr; pl->d.band_lo = nullptr; pl->d.row_scale = nullptr;
    const int rs = pl->rsize(), cs = pl->csize();
    const int64_t nnz = d.band_off[d.na];
    DeviceArena& mem = pl->mem;
    int rc;
    if ((rc = mem.upload(&pl->bank, d.bank, (size_t)nnz * rs))) return rc;
    if ((rc = mem.upload(&pl->band_off, d.band_off, (size_t)(d.na + 1) * 8))) return rc;
    if ((rc = mem.upload(&pl->band_lo, d.band_lo, (size_t)d.na * 4))) return rc;
    if (d.row_scale && (rc = mem.upload(&pl->row_scale, d.row_scale, (size_t)d.na * rs))) return rc;
    if ((rc = mem.alloc(&pl->xp, (size_t)pl->d.max_batch * d.m * rs))) return rc;
    if ((rc = mem.alloc(&pl->xh, (size_t)pl->d.max_batch * (d.m / 2 + 1) * cs))) return rc;
    // product workspace: 2 planes (Wx, dWx) per row, bounded to ~2 GiB
    const size_t per_row = (size_t)2 * d.m * cs;
    const size_t budget = (size_t)2 << 30;
    pl->rows_chunk = std::max<int64_t>(1, std::min<int64_t>(d.na, (int64_t)(budget / per_row)));
    // (allocated by the first execute that sends rows through the generic route: a plan whose rows all run on the
    // block / tile kernels -- the usual case -- never needs these up to 2 GiB)
    pl->prod_bytes = (size_t)pl->rows_chunk * per_row;
    {
        // default: up to 16 signals per launch (measured at config 2: 16 -> +1 % over 8), bin maps
        // bounded to ~2 GiB
        const int64_t g = std::min<int64_t>(16, std::max<int64_t>(1, ((int64_t)1 << 30) / (d.na * d.n)));
        pl->group = (int)std::max<int64_t>(1, std::min<int64_t>(g, pl->d.max_batch));
    }
    if ((rc = mem.alloc(&pl->kidx, ((size_t)pl->group * d.na * d.n + 64) * 2))) return rc;
    {
        std::vector<int32_t> all((size_t)d.na);
        for (int64_t i = 0; i < d.na; ++i) all[i] = (int32_t)i;
        if ((rc = mem.upload(&pl->gen_rows, all.data(), (size_t)d.na * 4))) return rc;
        if ((rc = mem.upload(&pl->all_rows, all.data(), (size_t)d.na * 4))) return rc;
        pl->n_gen = d.na;
    }
    if ((rc = pl->fwd.create(0, d.dtype, (size_t)d.m, (size_t)pl->d.max_batch, 1.0))) return rc;
    *out = pl.release();
    return 0;
}

void ssq_cwt_plan_destroy(ssq_cwt_plan* pl) {
    if (!pl) return;
    pl->fwd.destroy();
    for (auto& kv : pl->inv) kv.second.destroy();
    for (auto& kv : pl->adj_fwd) kv.second.destroy();
    if (pl->blk) destroy_blocks(pl->blk);
    if (pl->tile) destroy_tiles(pl->tile);
    pl->timer.destroy();
    pl->weights.destroy();
    pl->order.destroy();
    pl->mem.release();
    delete pl;
}

int ssq_cwt_plan_set_ssq(ssq_cwt_plan* pl, int grid, const double* params, const void* cst,
                         int cst_f64, int flipud, double gamma) {
    SSQ_REQUIRE(pl && params && cst, "ssq_cwt_plan_set_ssq: null pointer");
    SSQ_REQUIRE(grid >= SSQ_GRID_LOG && grid <= SSQ_GRID_LIN, "unknown grid kind %d", grid);
    std::lock_guard<std::mutex> lock(pl->order.mu);
    int rc = set_ssq_params(pl->sp, pl->weights, &pl->cst, &pl->cst0, pl->d.dtype, pl->d.na, grid, params, cst, cst_f64,
                            flipud, gamma);
    if (rc) return rc;
    pl->have_ssq = true;
    return 0;
}

int ssq_cwt_plan_set_blocks(ssq_cwt_plan* pl, const ssq_cwt_blocks_desc* bd) {
    SSQ_REQUIRE(pl && bd, "ssq_cwt_plan_set_blocks: null pointer");
    SSQ_REQUIRE(!pl->executed && !pl->blk, "block tables must be set once, before the first execute");
    SSQ_REQUIRE(pl->d.padtype != SSQ_PAD_NONE, "the block path needs a padded (power-of-two) length");
    SSQ_REQUIRE((pl->d.m & (pl->d.m - 1)) == 0, "the block path needs a power-of-two padded length");
    SSQ_REQUIRE(bd->n_classes >= 1 && bd->n_generic >= 0 && bd->n_generic <= pl->d.na, "bad block tables");
    for (int c = 0; c < bd->n_classes; ++c) {
        int64_t P = bd->classes[5 * c];
        SSQ_REQUIRE(P >= 4096 && (P & (P - 1)) == 0 && P <= pl->d.m, "class %d: bad block length %lld", c, (long long)P);
    }
    PlanGuard<BlockPlan> b(new BlockPlan(), destroy_blocks);
    b->group = pl->group;
    int rc = b->create(*bd, pl->d.dtype, pl->d.m, pl->d.n, pl->d.n1, pl->d.na, pl->d.max_batch);
    if (rc) return rc;
    if (bd->n_generic && pl->d.dtype == SSQ_F32) {      // four-step exact kernels: float32 only
        std::vector<int32_t> hg(bd->generic_rows, bd->generic_rows + bd->n_generic);
        rc = b->setup_exact((const float*)pl->bank, pl->band_off, pl->band_lo, pl->gen_rows,
                            pl->h_band_off, pl->h_band_lo, hg);
        if (rc) return rc;
    }
    if (bd->n_generic)
        SSQ_CHECK_HIP(hipMemcpy(pl->gen_rows, bd->generic_rows, (size_t)bd->n_generic * 4, hipMemcpyHostToDevice));
    pl->n_gen = bd->n_generic;
    pl->algo = !pl->n_gen ? "blockzoom" : (b->exact_ok ? "blockzoom+fourstep" : "blockzoom+rocfft");
    pl->blk = b.release();
    return 0;
}

int ssq_cwt_plan_set_tiles(ssq_cwt_plan* pl, const ssq_cwt_tiles_desc* td) {
    SSQ_REQUIRE(pl && td, "ssq_cwt_plan_set_tiles: null pointer");
    SSQ_REQUIRE(pl->blk && !pl->executed && !pl->tile,
                "tile tables must be set once, after the block tables, before the first execute");
    SSQ_REQUIRE(pl->d.dtype == SSQ_F32, "the tile path is float32 only");
    for (int t = 0; t < 5; ++t)
        SSQ_REQUIRE(td->n_items_tile[t] >= 0 && td->n_items_tile[t] <= pl->blk->n_items[t],
                    "tile tables: bad block item count in slot %d", t);
    PlanGuard<TilePlan> tp(new TilePlan(), destroy_tiles);
    int rc = tp->create(*td, pl->d.m, pl->d.n, pl->d.n1, pl->d.na, pl->group, pl->d.dt);
    if (rc) return rc;
    tp->class_need.assign((size_t)pl->blk->nc, 0);
    for (int t = 0; t < 5; ++t)
        for (int64_t q = 0; q < td->n_items_tile[t]; ++q) {
            const int c = pl->blk->h_items[t][4 * q + 3];
            if (c >= 0 && c < pl->blk->nc) tp->class_need[(size_t)c] = 1;
        }
    pl->tile = tp.release();
    pl->algo += "+tiles";
    return 0;
}

int ssq_cwt_plan_timing(ssq_cwt_plan* pl, int enable, double* stage_ms, int64_t* signals) {
    SSQ_REQUIRE(pl, "ssq_cwt_plan_timing: null plan");
    if (stage_ms) for (int t = 0; t < 4; ++t) stage_ms[t] = pl->timer.stage_ms[t];
    if (signals) *signals = pl->timer.signals;
    if (enable >= 0) pl->timer.reset(enable != 0);
    return 0;
}

int ssq_cwt_plan_set_bin_dump(ssq_cwt_plan* pl, unsigned short* kmap) {
    SSQ_REQUIRE(pl, "ssq_cwt_plan_set_bin_dump: null plan");
    std::lock_guard<std::mutex> lock(pl->order.mu);
    pl->kdump = kmap;
    return 0;
}

int ssq_cwt_plan_group(const ssq_cwt_plan* pl) { return pl ? pl->group : 0; }
int ssq_cwt_tile_rows_per_step(void) { return ssq::tile_rows_per_step(); }
int64_t ssq_cwt_plan_tiles_done(ssq_cwt_plan* pl, void* stream) {
    if (!pl || !pl->tile) return 0;
    return pl->tile->tiles_done(as_stream(stream));
}
int ssq_cwt_plan_tile_cols(const ssq_cwt_plan* pl) { return (pl && pl->tile) ? pl->tile->tile_cols() : 0; }
int ssq_cwt_plan_tile_counters(ssq_cwt_plan* pl, unsigned long long* out, int n, void* stream) {
    SSQ_REQUIRE(pl && out && n >= 0 && n <= 512, "ssq_cwt_plan_tile_counters: bad arguments");
    memset(out, 0, (size_t)n * 8);
    if (!pl->tile || !pl->tile->counters) return 0;
    SSQ_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    SSQ_CHECK_HIP(hipMemcpy(out, pl->tile->counters, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}
int ssq_cwt_plan_tile_kernel(const ssq_cwt_plan* pl) { return (pl && pl->tile) ? pl->tile->tile_kernel() : 0; }
int64_t ssq_cwt_plan_bytes(const ssq_cwt_plan* pl) { return pl ? pl->bytes() : 0; }
const char* ssq_cwt_plan_algo(const ssq_cwt_plan* pl) { return pl ? pl->algo.c_str() : ""; }

}  // extern "C"

// ---- one execute: its arguments, what it decides before any row is routed, and its stages ---------------------------
struct CwtCall {
    ssq_cwt_plan* pl;
    const void* x; int64_t batch;
    void* Wx; void* dWx; void* Tx; void* w;
    int rpadded;
    hipStream_t stream;
    bool use_blocks = false;      // the block (+ exact) kernels take the rows they can
    bool use_tiles = false;       // fused ssq form on the column-tile path: block / exact kernels only for the rows the
                                  // tile kernel reads back, no separate reassignment launch
    bool side = false;            // ... with the decimated samples on the tile plan's side stream
    int64_t n_gen = 0;            // rows of the exact / generic route
    unsigned short* kidx = nullptr;   // the bin map, where the reassignment reads one
    int64_t out_cols() const { return rpadded ? pl->d.m : pl->d.n; }
    int nplanes() const { return (dWx || Tx || w) ? 2 : 1; }
};

// pad (or copy) the whole batch, forward FFT of all signals at once
// (a smaller batch than planned runs the planned batch over the valid prefix; rows past `batch` hold stale but finite
// data and are ignored)
static int cwt_pad_fft(const CwtCall& c) {
    ssq_cwt_plan* pl = c.pl;
    const ssq_cwt_desc& d = pl->d;
    if (d.padtype != SSQ_PAD_NONE) {
        int rc = ssq_pad_signal(d.dtype, c.x, pl->xp, c.batch, d.n, d.n1, d.m - d.n - d.n1, d.padtype, c.stream);
        if (rc) return rc;
    } else
        SSQ_CHECK_HIP(hipMemcpyAsync(pl->xp, c.x, (size_t)c.batch * d.m * pl->rsize(), hipMemcpyDeviceToDevice, c.stream));
    return pl->fwd.execute(pl->xp, pl->xh, c.stream);
}

// Decimated samples of the interpolated rows of signals b0 .. b0 + ng - 1 (tile path). With the side stream: forked
// from the execute's stream -- which also orders this group's samples behind the previous group's tile kernel -- and
// left to be joined by cwt_reassign; when timing stage by stage they run in line.
static int cwt_tile_samples(const CwtCall& c, int64_t b0, int ng) {
    TilePlan* t = c.pl->tile;
    hipStream_t ss = c.side ? t->side : c.stream;
    if (c.side) {
        SSQ_CHECK_HIP(hipEventRecord(t->ev_fork, c.stream));
        SSQ_CHECK_HIP(hipStreamWaitEvent(ss, t->ev_fork, 0));
    }
    int rc = t->spectra((int)b0, ng, c.pl->xh, ss);
    if (rc) return rc;
    if (c.side) SSQ_CHECK_HIP(hipEventRecord(t->ev_join, ss));
    return 0;
}

template <typename T>
static int cwt_block_rows(const CwtCall& c, int64_t b0, int ng) {
    ssq_cwt_plan* pl = c.pl;
    if constexpr (sizeof(T) == 4)
        return pl->blk->run((int)b0, ng, (float*)c.Wx, (float*)c.dWx, (float*)c.w, c.kidx, (const float*)pl->row_scale,
                            pl->d.dt, pl->sp, c.stream, c.use_tiles ? pl->tile->n_items_tile : nullptr);
    else
        return pl->blk->run64((int)b0, ng, (double*)c.Wx, (double*)c.dWx, (double*)c.w, c.kidx,
                              (const double*)pl->row_scale, pl->d.dt, pl->sp, c.stream);
}

// the rows whose band is cut by the Nyquist bin, four-step full-length FFT (float32), the whole group in one launch
// (sub-groups of n signals, so that the four-step intermediate Z -- 4 MB per row and signal -- could stay
// in the 256 MiB Infinity Cache between the two passes, were measured on the MI355X at config 2: 16 signals
// at once 68.9 us per transform, 4: 76.2, 2: 73.7, 1: 85.3 -- the cache does not pay for the smaller launches)
static int cwt_exact_rows(const CwtCall& c, int64_t b0, int ng) {
    ssq_cwt_plan* pl = c.pl;
    return pl->blk->run_exact((int)b0, ng, pl->xh, (float*)c.Wx, (float*)c.dWx, (float*)c.w, c.kidx,
                              (const float*)pl->row_scale, pl->d.dt, pl->sp, c.stream);
}

// generic route, signal by signal in row chunks: banded product, rocFFT inverse (the plans cached by their transform
// count), epilogue; the product workspace exists from the first execute that sends rows here
template <typename T>
static int cwt_generic_rows(const CwtCall& c, int64_t b0, int ng) {
    ssq_cwt_plan* pl = c.pl;
    const ssq_cwt_desc& d = pl->d;
    const int64_t M = d.m, N = d.n, na = d.na, out_cols = c.out_cols(), n_gen = c.n_gen;
    const int nplanes = c.nplanes();
    const double h = (2.0 * 3.141592653589793) / (double)M;
    const T inv_dt = T(1) / (T)d.dt;
    const int32_t* rowlist = pl->gen_rows_for(c.use_blocks);
    if (n_gen > 0) {
        int rc = cwt_product_workspace(pl);
        if (rc) return rc;
    }
    for (int64_t b = b0; b < b0 + ng; ++b) {
        const T* xh = (const T*)pl->xh + (size_t)b * (M / 2 + 1) * 2;
        for (int64_t row0 = 0; row0 < n_gen; row0 += pl->rows_chunk) {
            const int64_t rows = std::min(pl->rows_chunk, n_gen - row0);
            unsigned gx = (unsigned)std::min<int64_t>((M + 255) / 256, 4096);
            hipLaunchKernelGGL((bank_multiply_kernel<T>), dim3(gx, (unsigned)rows), dim3(256), 0, c.stream,
                               xh, (const T*)pl->bank, pl->band_off, pl->band_lo, (T*)pl->prod, M,
                               rowlist, row0, nplanes, h, inv_dt);
            SSQ_LAUNCH_CHECK();
            int rc = cwt_cached_fft(pl, pl->inv, 1, rows * nplanes, 1.0 / (double)M, pl->prod, c.stream);
            if (rc) return rc;
            EpilogueArgs ea;
            ea.Wx = c.Wx ? (T*)c.Wx + (size_t)b * na * out_cols * 2 : nullptr;
            ea.dWx = c.dWx ? (T*)c.dWx + (size_t)b * na * out_cols * 2 : nullptr;
            ea.w = c.w ? (T*)c.w + (size_t)b * na * out_cols : nullptr;
            ea.kidx = c.kidx ? c.kidx + (size_t)(b - b0) * na * N : nullptr;
            ea.out_cols = out_cols; ea.col0 = c.rpadded ? 0 : d.n1; ea.row0 = row0;
            ea.rowlist = rowlist;
            ea.row_scale = pl->row_scale; ea.gamma = pl->sp.gamma; ea.have_ssq = pl->have_ssq;
            unsigned ex = (unsigned)std::min<int64_t>((out_cols + 255) / 256, 4096);
            hipLaunchKernelGGL((cwt_epilogue_kernel<T>), dim3(ex, (unsigned)rows), dim3(256), 0, c.stream,
                               (const T*)pl->prod, M, nplanes, na, ea, pl->sp);
            SSQ_LAUNCH_CHECK();
        }
    }
    return 0;
}

// Tx of the group: the tile kernel (joins the side stream first; also writes Wx of the interpolated rows), or the
// separate reassignment from the bin map / w
template <typename T>
static int cwt_reassign(const CwtCall& c, int64_t b0, int ng) {
    ssq_cwt_plan* pl = c.pl;
    const int64_t N = pl->d.n, na = pl->d.na, out_cols = c.out_cols();
    if (c.use_tiles) {
        if (c.side) SSQ_CHECK_HIP(hipStreamWaitEvent(c.stream, pl->tile->ev_join, 0));
        return pl->tile->run((int)b0, ng, (float*)c.Wx, (float*)c.dWx, (float*)c.Tx, pl->kidx, pl->cst, pl->cst0, pl->sp,
                             c.stream, pl->kdump);
    }
    if (!c.Tx) return 0;
    // (diagnostic: the map the separate reassignment is about to consume)
    if (pl->kdump && !c.w)
        SSQ_CHECK_HIP(hipMemcpyAsync(pl->kdump + (size_t)b0 * na * N, pl->kidx, (size_t)ng * na * N * 2,
                                     hipMemcpyDeviceToDevice, c.stream));
    T* Wx_g = (T*)c.Wx + (size_t)b0 * na * out_cols * 2;
    T* w_g = c.w ? (T*)c.w + (size_t)b0 * na * out_cols : nullptr;
    T* Tx_g = (T*)c.Tx + (size_t)b0 * na * out_cols * 2;
    return launch_accumulate(pl->d.dtype, c.w ? BIN_FROM_W : BIN_FROM_KIDX, Wx_g,
                             c.w ? (const void*)w_g : (const void*)pl->kidx, nullptr, Tx_g,
                             pl->cst, pl->sp, ng, na, N, nullptr, c.stream);
}

template <typename T>
static int cwt_execute_t(CwtCall& c) {
    ssq_cwt_plan* pl = c.pl;
    StageTimer& tm = pl->timer;
    const int64_t batch = c.batch;
    int rc = tm.begin((batch + pl->group - 1) / pl->group, c.stream);
    if (rc) return rc;
    if ((rc = cwt_pad_fft(c))) return rc;
    pl->executed = true;
    c.use_blocks = pl->blk && !c.rpadded;
    c.n_gen = c.use_blocks ? pl->n_gen : pl->d.na;
    // (a tile plan the selected kernel cannot run -- more rows than the ordered kernel's tile holds -- is decided
    // HERE, before any row is routed: those calls take the block kernels + the separate reassignment)
    c.use_tiles = c.use_blocks && pl->tile && pl->tile->usable() && c.Tx && !c.w && sizeof(T) == 4;
    c.side = c.use_tiles && pl->tile->side && !tm.on;
    c.kidx = (c.Tx && !c.w) ? pl->kidx : nullptr;
    // The first launch group's decimated samples need the spectra xh and nothing else: their kernels go to the side stream
    // HERE, beside the analytic signal and the block spectra, not only beside the block rows (a short signal's ssq_cwt:
    // their three launches are the longer branch).
    if (c.side && (rc = cwt_tile_samples(c, 0, (int)std::min<int64_t>(pl->group, batch)))) return rc;
    if (c.use_blocks && (rc = pl->blk->spectra(pl->xp, pl->xh, batch, c.stream, c.use_tiles ? pl->tile->class_need.data() : nullptr)))
        return rc;
    tm.front_done();
    int64_t g = 0;                                      // launch group = timing slot
    for (int64_t b0 = 0; b0 < batch; b0 += pl->group, ++g) {
        const int ng = (int)std::min<int64_t>(pl->group, batch - b0);
        if (c.use_tiles && !(c.side && b0 == 0)) {      // counted with stage 0
            tm.mark(g, StageTimer::SAMPLES);
            if ((rc = cwt_tile_samples(c, b0, ng))) return rc;
            tm.mark(g, StageTimer::SAMPLES_END);
        }
        tm.mark(g, StageTimer::ROWS);
        if (c.use_blocks && (rc = cwt_block_rows<T>(c, b0, ng))) return rc;
        tm.mark(g, StageTimer::OTHER_ROWS);
        const bool exact = c.use_blocks && pl->blk->exact_ok && c.n_gen > 0;      // (exact_ok: float32 plans only)
        if ((rc = exact ? cwt_exact_rows(c, b0, ng) : cwt_generic_rows<T>(c, b0, ng))) return rc;
        tm.mark(g, StageTimer::REASSIGN);
        if ((rc = cwt_reassign<T>(c, b0, ng))) return rc;
        tm.mark(g, StageTimer::GROUP_END);
    }
    return tm.finish(g, c.use_tiles, batch);
}

extern "C" {

int ssq_cwt_execute(ssq_cwt_plan* pl, const void* x, int64_t batch, void* Wx, void* dWx, void* Tx,
                    void* w, int rpadded, void* stream) {
    SSQ_REQUIRE(pl && x, "ssq_cwt_execute: null pointer");
    SSQ_REQUIRE(batch >= 1 && batch <= pl->d.max_batch, "batch %lld outside [1, %lld]",
                (long long)batch, (long long)pl->d.max_batch);
    SSQ_REQUIRE(Wx || !(dWx || Tx || w), "Wx buffer is required");
    SSQ_REQUIRE(!(rpadded && (Tx || w)), "rpadded output excludes Tx / w");
    SSQ_REQUIRE(!Tx || pl->have_ssq, "Tx requested but ssq parameters were not set");
    SSQ_REQUIRE(!w || pl->have_ssq, "w requested but ssq parameters (gamma) were not set");
    SSQ_REQUIRE(Wx, "Wx buffer is required");
    hipStream_t st = as_stream(stream);
    pl->order.enter(st);
    // (replaying the launches of small transforms from a hipGraph was built in round 2 and
    // measured slower than the eager launches on ROCm 7.2 -- config 1: 0.298 vs 0.126 ms -- so it
    // is gone; what helps small transforms is fewer launches)
    CwtCall c{pl, x, batch, Wx, dWx, Tx, w, rpadded, st};
    const int rc = dispatch_dtype(pl->d.dtype, [&](auto t) { return cwt_execute_t<decltype(t)>(c); });
    pl->order.leave(st);
    return rc;
}

}  // extern "C"

// ---- adjoint of the plan's CWT (ssq_cwt_adjoint): gWx, gdWx -> gx --------------------------------------------------
// With F_a = fft_M(U gWx_a), G_a = fft_M(U gdWx_a) (U: the n columns at offset n1 of a zero row of length M):
//   gx = pad^T Re ifft_M( sum_a s_a psi_a[k] (F_a[k] - i m_k G_a[k]) )
// Per signal and pass of rows (the forward's rows_chunk cut to ADJ_PASS_BYTES, in the forward's product workspace):
//   gWx, gdWx --cwt_adjoint_stage_kernel--> zero-extended rows --rocFFT C2C forward, batched, in place-->
//   --cwt_adjoint_mac_kernel--> the signal's spectrum sum (adds to what the earlier passes left)
// then for the whole batch: rocFFT C2C inverse (1/M) of the spectrum sums --cwt_adjoint_unpad_kernel--> gx.
// Every sum has one order (rows ascending per bin, padded positions ascending per sample): the same input gives the same
// bits, whatever the batch.
namespace ssq {

constexpr int ADJ_SEG = 512;       // bins per entry of the row-range table (a multiple of a workgroup's bins)
constexpr size_t ADJ_PASS_BYTES = (size_t)128 << 20;   // rows staged, transformed and summed per pass

// ws[r][p][k] = g_p[row0 + r][k - col0] for col0 <= k < col0 + cols, else 0: a work-item writes V bins, 16 bytes a store
// (V = 2 complex64 / 1 complex128; V = 1 with 8-byte stores for complex64 rows of an odd length M)
template <typename T, int V>
__global__ __launch_bounds__(256) void cwt_adjoint_stage_kernel(const T* __restrict__ g0, const T* __restrict__ g1,
                                                                T* __restrict__ ws, int64_t M, int64_t cols, int64_t col0,
                                                                int64_t row0, int nplanes) {
    typedef T vec_t __attribute__((ext_vector_type(2 * V)));
    typedef T cx_t __attribute__((ext_vector_type(2)));
    const int64_t r = blockIdx.y;
    const int p = blockIdx.z;
    const T* g = (p ? g1 : g0) + 2 * (row0 + r) * cols;
    T* o = ws + 2 * ((r * nplanes + p) * M);
    for (int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V; k < M;
         k += (int64_t)gridDim.x * blockDim.x * V) {                 // (V == 2 only where M is even: k + 1 < M)
        vec_t out;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t j = k + v - col0;
            cx_t c = {T(0), T(0)};
            if (j >= 0 && j < cols) c = *reinterpret_cast<const cx_t*>(g + 2 * j);
            out[2 * v] = c[0]; out[2 * v + 1] = c[1];
        }
        *reinterpret_cast<vec_t*>(o + 2 * k) = out;
    }
}

// S[k] += sum over the rows a of the chunk whose band holds k, ascending, of s_a psi_a[k] (F_a[k] - i m_k G_a[k]).
// A work-item owns V neighbouring bins; `seg` holds, per ADJ_SEG bins, the first row and one past the last row whose
// band reaches the segment: a workgroup walks only those, and one whose segment no row of the chunk reaches -- every
// bin above M/2 of an analytic bank -- returns without reading anything. F, G: planes of the workspace
// [rows][planes][M], 16 bytes a load where V == 2; the bank is the plan's banded one.
template <typename T, int V, bool HAS_F, bool HAS_G>
__global__ __launch_bounds__(256) void cwt_adjoint_mac_kernel(
    const T* __restrict__ ws, const T* __restrict__ bank, const int64_t* __restrict__ band_off,
    const int32_t* __restrict__ band_lo, const T* __restrict__ row_scale, const int32_t* __restrict__ seg,
    T* __restrict__ S, int64_t M, int64_t row0, int64_t rows, double h, T inv_dt) {
    typedef T vec_t __attribute__((ext_vector_type(2 * V)));
    constexpr int NP = (HAS_F ? 1 : 0) + (HAS_G ? 1 : 0);
    const int64_t kb = (int64_t)blockIdx.x * blockDim.x * V;        // first bin of the workgroup
    const int64_t sg = kb / ADJ_SEG;
    const int64_t s_lo = seg[2 * sg], s_hi = seg[2 * sg + 1];
    const int64_t a_lo = s_lo > row0 ? s_lo : row0, a_hi = s_hi < row0 + rows ? s_hi : row0 + rows;
    const int64_t k0 = kb + (int64_t)threadIdx.x * V;
    if (a_lo >= a_hi || k0 >= M) return;
    T mk[V], re[V], im[V];
    vec_t acc = *reinterpret_cast<const vec_t*>(S + 2 * k0);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        // the forward's derivative multiplier, as bank_multiply_kernel forms it
        const int64_t k = k0 + v, ks = k <= M / 2 ? k : k - M;
        mk[v] = (T)((double)ks * h) * inv_dt;
        re[v] = acc[2 * v]; im[v] = acc[2 * v + 1];
    }
#pragma unroll 4
    for (int64_t a = a_lo; a < a_hi; ++a) {
        const int64_t lo = band_lo[a], off = band_off[a], len = band_off[a + 1] - off;
        if (len <= 0) continue;
        const T* P = ws + 2 * ((a - row0) * NP * M + k0);
        vec_t f, g;
        if (HAS_F) f = *reinterpret_cast<const vec_t*>(P);
        if (HAS_G) g = *reinterpret_cast<const vec_t*>(P + (HAS_F ? 2 * M : 0));
        const T s = row_scale ? row_scale[a] : T(1);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int64_t t = k0 + v - lo;
            const bool in = t >= 0 && t < len;
            T c = bank[off + (t < 0 ? 0 : (t < len ? t : len - 1))];
            if (row_scale) c = c * s;
            T tr = T(0), ti = T(0);
            if (HAS_F) { tr = f[2 * v]; ti = f[2 * v + 1]; }
            if (HAS_G) {                     // -i m (gr + i gi) = m gi - i m gr
                const T dr = mk[v] * g[2 * v + 1], di = -(mk[v] * g[2 * v]);
                tr = HAS_F ? tr + dr : dr; ti = HAS_F ? ti + di : di;
            }
            if (in) { re[v] = re[v] + c * tr; im[v] = im[v] + c * ti; }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) { acc[2 * v] = re[v]; acc[2 * v + 1] = im[v]; }
    *reinterpret_cast<vec_t*>(S + 2 * k0) = acc;
}

// gx[b][j] = sum over the padded positions p that copy sample j, ascending, of Re S[b][p]
template <typename T>
__global__ __launch_bounds__(256) void cwt_adjoint_unpad_kernel(const T* __restrict__ S, T* __restrict__ gx,
                                                                const int32_t* __restrict__ off,
                                                                const int32_t* __restrict__ idx, int64_t n, int64_t M) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const T* s = S + 2 * (int64_t)blockIdx.y * M;
    T acc = T(0);
    for (int32_t e = off[j]; e < off[j + 1]; ++e) acc = acc + s[2 * (int64_t)idx[e]];
    gx[(int64_t)blockIdx.y * n + j] = acc;
}

}  // namespace ssq

// the adjoint's tables and its spectrum buffer, at the first call
static int cwt_adjoint_setup(ssq_cwt_plan* pl) {
    if (pl->adj_spec) return 0;
    const ssq_cwt_desc& d = pl->d;
    SSQ_REQUIRE(d.m < ((int64_t)1 << 31), "cwt adjoint: padded length %lld", (long long)d.m);
    std::vector<int32_t> off, idx;
    inverse_pad_table(d.n, d.m, d.n1, d.padtype, off, idx);
    const int64_t nseg = (d.m + ADJ_SEG - 1) / ADJ_SEG;
    std::vector<int32_t> seg((size_t)(2 * nseg), 0);
    for (int64_t a = 0; a < d.na; ++a) {
        const int64_t lo = pl->h_band_lo[(size_t)a], len = pl->h_band_off[(size_t)a + 1] - pl->h_band_off[(size_t)a];
        if (len <= 0) continue;
        for (int64_t s = lo / ADJ_SEG; s <= (lo + len - 1) / ADJ_SEG; ++s) {
            int32_t* e = &seg[(size_t)(2 * s)];
            if (e[1] == 0) { e[0] = (int32_t)a; e[1] = (int32_t)a + 1; }
            else { e[0] = std::min(e[0], (int32_t)a); e[1] = std::max(e[1], (int32_t)a + 1); }
        }
    }
    // (a failure part-way is undone by ssq_cwt_adjoint, with whatever else its first call allocated)
    int rc = pl->mem.upload(&pl->adj_off, off.data(), off.size() * 4);
    if (!rc) rc = pl->mem.upload(&pl->adj_idx, idx.data(), idx.size() * 4);
    if (!rc) rc = pl->mem.upload(&pl->adj_seg, seg.data(), seg.size() * 4);
    if (!rc) rc = pl->mem.alloc(&pl->adj_spec, (size_t)d.max_batch * d.m * pl->csize());
    return rc;
}

template <typename T, int V>
static int cwt_adjoint_t(ssq_cwt_plan* pl, const void* gWx, const void* gdWx, void* gx, int64_t batch, int rpadded,
                         hipStream_t stream) {
    const ssq_cwt_desc& d = pl->d;
    const int64_t M = d.m, N = d.n, na = d.na;
    const int64_t cols = rpadded ? M : N, col0 = rpadded ? 0 : d.n1;
    const int nplanes = (gWx ? 1 : 0) + (gdWx ? 1 : 0);
    const double h = (2.0 * 3.141592653589793) / (double)M;
    const T inv_dt = T(1) / (T)d.dt;
    int rc = cwt_product_workspace(pl);
    if (rc) return rc;
    T* ws = (T*)pl->prod;
    // rows per pass: the forward's chunk, cut to ADJ_PASS_BYTES of rows (two planes each) -- rocFFT's own work area
    // is as large as what it transforms in one call, and a pass of this size is still in the Infinity Cache when the
    // next kernel reads it
    // (measured at N = 160 000, 300 scales, one signal, gWx alone / with gdWx: 32 MiB 1.80 / 2.78 ms, 128 MiB 1.34 / 2.39,
    // 512 MiB 1.35 / 2.68, all rows at once 1.34 / 3.07)
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(pl->rows_chunk,
                                                                 (int64_t)(ADJ_PASS_BYTES / ((size_t)4 * M * sizeof(T)))));
    SSQ_CHECK_HIP(hipMemsetAsync(pl->adj_spec, 0, (size_t)batch * M * 2 * sizeof(T), stream));
    const unsigned sx = (unsigned)std::min<int64_t>((M + 256 * V - 1) / (256 * V), 4096);
    const unsigned mx = (unsigned)((M + 256 * V - 1) / (256 * V));
    for (int64_t b = 0; b < batch; ++b) {
        const T* g0 = (const T*)(gWx ? gWx : gdWx) + (size_t)b * na * cols * 2;
        const T* g1 = (gWx && gdWx) ? (const T*)gdWx + (size_t)b * na * cols * 2 : nullptr;
        T* S = (T*)pl->adj_spec + (size_t)b * M * 2;
        // (the workspace holds two planes per row of the chunk: whichever gradients are given fit)
        for (int64_t row0 = 0; row0 < na; row0 += chunk) {
            const int64_t rows = std::min(chunk, na - row0);
            hipLaunchKernelGGL((cwt_adjoint_stage_kernel<T, V>), dim3(sx, (unsigned)rows, (unsigned)nplanes), dim3(256), 0,
                               stream, g0, g1, ws, M, cols, col0, row0, nplanes);
            SSQ_LAUNCH_CHECK();
            rc = cwt_cached_fft(pl, pl->adj_fwd, 2, rows * nplanes, 1.0, ws, stream);
            if (rc) return rc;
#define SSQ_MAC(F, G) hipLaunchKernelGGL((cwt_adjoint_mac_kernel<T, V, F, G>), dim3(mx), dim3(256), 0, stream,           \
                                         (const T*)ws, (const T*)pl->bank, pl->band_off, pl->band_lo,                      \
                                         (const T*)pl->row_scale, (const int32_t*)pl->adj_seg, S, M, row0, rows, h, inv_dt)
            if (gWx && gdWx) SSQ_MAC(true, true);
            else if (gWx) SSQ_MAC(true, false);
            else SSQ_MAC(false, true);
#undef SSQ_MAC
            SSQ_LAUNCH_CHECK();
        }
    }
    rc = cwt_cached_fft(pl, pl->inv, 1, batch, 1.0 / (double)M, pl->adj_spec, stream);
    if (rc) return rc;
    hipLaunchKernelGGL((cwt_adjoint_unpad_kernel<T>), dim3((unsigned)((N + 255) / 256), (unsigned)batch), dim3(256), 0,
                       stream, (const T*)pl->adj_spec, (T*)gx, (const int32_t*)pl->adj_off, (const int32_t*)pl->adj_idx,
                       N, M);
    SSQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int ssq_cwt_adjoint(ssq_cwt_plan* pl, const void* gWx, const void* gdWx, void* gx, int64_t batch,
                               int rpadded, void* stream) {
    SSQ_REQUIRE(pl && gx, "ssq_cwt_adjoint: null pointer");
    SSQ_REQUIRE(gWx || gdWx, "ssq_cwt_adjoint: gWx and gdWx are both null");
    SSQ_REQUIRE(batch >= 1 && batch <= pl->d.max_batch, "batch %lld outside [1, %lld]",
                (long long)batch, (long long)pl->d.max_batch);
    SSQ_REQUIRE(batch <= 65535, "ssq_cwt_adjoint: batch %lld > 65535", (long long)batch);
    hipStream_t st = as_stream(stream);
    pl->order.enter(st);
    const bool first = !pl->adj_spec, had_prod = pl->prod != nullptr;
    const size_t before = pl->mem.count();
    int rc = cwt_adjoint_setup(pl);
    if (!rc) {
        if (pl->d.dtype == SSQ_F64) rc = cwt_adjoint_t<double, 1>(pl, gWx, gdWx, gx, batch, rpadded, st);
        else if (pl->d.m % 2 == 0) rc = cwt_adjoint_t<float, 2>(pl, gWx, gdWx, gx, batch, rpadded, st);
        else rc = cwt_adjoint_t<float, 1>(pl, gWx, gdWx, gx, batch, rpadded, st);
    }
    if (rc && first) {       // a first call that fails leaves the plan as it found it: the next one starts over
        pl->mem.release(before);
        pl->adj_off = pl->adj_idx = pl->adj_seg = nullptr; pl->adj_spec = nullptr;
        if (!had_prod) pl->prod = nullptr;
    }
    pl->order.leave(st);
    return rc;
}
