// plan_host_check.cpp -- the plans' device-memory owner (csrc/ssq_common.h: DeviceArena) and the helper both set_ssq
// entries call (set_ssq_params), driven on the host against the emulator's headers (tests/emu/hip), with hipMalloc,
// hipFree and hipMemcpy counted here. A program of its own: tests/test_plan_host_layer.py builds it with
// -fsanitize=address,undefined and runs it. TEST INFRASTRUCTURE ONLY.
#include "hip/hip_runtime.h"
#include <map>

static std::map<void*, size_t> g_live;         // what counted_malloc handed out and nobody freed yet, with its size
static int g_mallocs = 0, g_frees = 0, g_bad_frees = 0, g_copies = 0, g_bad_copies = 0, g_fail_malloc_at = 0;

static hipError_t counted_malloc(void** p, size_t n) {
    if (++g_mallocs == g_fail_malloc_at) { *p = nullptr; return 2; }
    if (n == 0) { *p = nullptr; return 1; }                  // (a caller must never ask the runtime for 0 bytes)
    *p = malloc(n);
    g_live[*p] = n;
    return hipSuccess;
}
static hipError_t counted_free(void* p) {
    if (!g_live.erase(p)) { ++g_bad_frees; return 1; }
    free(p);
    ++g_frees;
    return hipSuccess;
}
static hipError_t counted_memcpy(void* d, const void* s, size_t n, int) {
    auto it = g_live.find(d);
    if (it == g_live.end() || it->second < n) { ++g_bad_copies; return 1; }
    if (n) memcpy(d, s, n);
    ++g_copies;
    return hipSuccess;
}
#define hipMalloc counted_malloc
#define hipFree counted_free
#define hipMemcpy counted_memcpy

#include "ssq_common.h"

namespace ssq {
static int g_errors = 0;
void set_error(const char*, ...) { ++g_errors; }
}

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

// ---- the arena: a plan's create in miniature -- uploads of these sizes, then one plain allocation
static const size_t SIZES[] = {40, 0, 8, 1024, 0, 12};
constexpr int N_UP = sizeof(SIZES) / sizeof(SIZES[0]);

static int uploads(ssq::DeviceArena& mem, void** ptrs) {
    static const unsigned char host[1024] = {1, 2, 3};
    for (int i = 0; i < N_UP; ++i) {
        const int rc = mem.upload(&ptrs[i], host, SIZES[i]);
        if (rc) return rc;
    }
    return mem.alloc(&ptrs[N_UP], 64);
}

static void check_arena() {
    {   // every allocation succeeds: the total is what was asked for, a size of 0 is a valid pointer of its own
        ssq::DeviceArena mem;
        void* ptrs[N_UP + 1] = {nullptr};
        CHECK(uploads(mem, ptrs) == 0 && g_mallocs == N_UP + 1 && (int)g_live.size() == N_UP + 1);
        CHECK(mem.bytes() == 40 + 8 + 1024 + 12 + 64 && mem.count() == (size_t)N_UP + 1);
        for (int i = 0; i <= N_UP; ++i) CHECK(ptrs[i] && g_live.count(ptrs[i]));
        CHECK(ptrs[1] != ptrs[4] && g_live[ptrs[1]] == 1);
        CHECK(g_copies == 4 && g_bad_copies == 0);           // (nothing is copied for a size of 0)
        CHECK(((unsigned char*)ptrs[0])[2] == 3);
        // a setup that fails part-way gives back what it took: the rest stays
        const size_t before = mem.count();
        void* extra = nullptr;
        CHECK(mem.alloc(&extra, 16) == 0 && mem.alloc(&extra, 32) == 0 && mem.bytes() == 1148 + 48);
        mem.release(before);
        CHECK(mem.count() == before && mem.bytes() == 1148 && (int)g_live.size() == N_UP + 1 && g_frees == 2);
        mem.release();
        CHECK(g_live.empty() && g_frees == N_UP + 3 && mem.bytes() == 0 && mem.count() == 0);
        mem.release();                                       // a second release frees nothing
        CHECK(g_frees == N_UP + 3 && g_bad_frees == 0);
    }
    // the k-th allocation fails: the call reports it, the total is what was handed out before, release frees exactly that
    for (int k = 1; k <= N_UP + 1; ++k) {
        g_mallocs = g_frees = 0; ssq::g_errors = 0;
        g_fail_malloc_at = k;
        ssq::DeviceArena mem;
        void* ptrs[N_UP + 1] = {nullptr};
        CHECK(uploads(mem, ptrs) == -2 && ssq::g_errors == 1 && g_mallocs == k);
        g_fail_malloc_at = 0;
        int64_t handed = 0;
        for (int i = 0; i < k - 1; ++i) handed += (int64_t)SIZES[i];
        CHECK(mem.bytes() == handed && mem.count() == (size_t)(k - 1) && (int)g_live.size() == k - 1);
        CHECK(ptrs[k - 1] == nullptr);                       // the failed request left a null pointer, not a stale one
        mem.release();
        CHECK(g_live.empty() && g_frees == k - 1);
        mem.release();
        CHECK(g_frees == k - 1 && g_bad_frees == 0);
    }
    CHECK(g_bad_copies == 0);
}

// ---- set_ssq_params: the uniform-weights scan by the weights' type, the first weight, and a float64 plan's masking
static const double LOG_PARAMS[5] = {-3.0, 0.05, 0, 0, 0};

static void check_set_ssq() {
    struct Case { int dtype, cst_f64; bool uniform; };
    const Case cases[] = {{SSQ_F32, 0, true}, {SSQ_F32, 0, false}, {SSQ_F32, 1, true}, {SSQ_F32, 1, false},
                          {SSQ_F64, 0, true}, {SSQ_F64, 0, false}, {SSQ_F64, 1, true}, {SSQ_F64, 1, false}};
    const int rows = 7;
    for (const Case& c : cases) {
        const bool wide = c.cst_f64 || c.dtype == SSQ_F64;
        // (as doubles the weights differ in the LAST row only, by one unit in the last place: rounded to float they
        // would be equal -- a scan that read them in the wrong type sees garbage or misses the difference)
        float wf[rows]; double wd[rows];
        for (int i = 0; i < rows; ++i) { wf[i] = 0.75f; wd[i] = 0.75; }
        if (!c.uniform) { wf[rows - 1] = 0.5f; wd[rows - 1] = 0.75 + 1.1102230246251565e-16; }
        ssq::SsqParams sp{};
        sp.cst_f64 = 7; sp.cst_uniform = 7;
        ssq::WeightVersions weights;
        void* dev = nullptr; float first = 0.f;
        const size_t live = g_live.size();
        const int rc = ssq::set_ssq_params(sp, weights, &dev, &first, c.dtype, rows, SSQ_GRID_LOG, LOG_PARAMS,
                                           wide ? (const void*)wd : (const void*)wf, c.cst_f64, 1, 0.25);
        CHECK(rc == 0 && sp.cst_uniform == (c.uniform ? 1 : 0) && first == 0.75f);
        CHECK(sp.cst_f64 == ((c.cst_f64 && c.dtype == SSQ_F32) ? 1 : 0));      // a float64 plan reads its own type
        CHECK(sp.grid == SSQ_GRID_LOG && sp.flipud == 1 && sp.gamma == 0.25 && sp.p[0] == -3.0 && sp.p[1] == 0.05);
        CHECK(sp.pf[0] == -3.0f && sp.pf[1] == (float)(1.0 / 0.05) && sp.guard > 0.f && sp.guard < 0.25f);
        CHECK(g_live.size() == live + 1 && dev && g_live[dev] == (size_t)rows * (wide ? 8 : 4));
        CHECK(memcmp(dev, wide ? (const void*)wd : (const void*)wf, (size_t)rows * (wide ? 8 : 4)) == 0);
        weights.destroy();
        CHECK(g_live.size() == live);
    }
    {   // one row is uniform; an unknown grid is refused before anything is uploaded
        ssq::SsqParams sp{};
        ssq::WeightVersions weights;
        void* dev = nullptr; float first = 0.f;
        const float one = 2.f;
        CHECK(ssq::set_ssq_params(sp, weights, &dev, &first, SSQ_F32, 1, SSQ_GRID_LIN, LOG_PARAMS, &one, 0, 0, 0.) == 0);
        CHECK(sp.cst_uniform == 1 && first == 2.f && sp.flipud == 0);
        const int mallocs = g_mallocs;
        CHECK(ssq::set_ssq_params(sp, weights, &dev, &first, SSQ_F32, 1, 99, LOG_PARAMS, &one, 0, 0, 0.) == -1);
        CHECK(g_mallocs == mallocs);
        weights.destroy();
        CHECK(g_live.empty());
    }
    CHECK(g_bad_frees == 0 && g_bad_copies == 0);
}

int main() {
    check_arena();
    check_set_ssq();
    printf(g_failed ? "FAIL\n" : "PASS\n");
    return g_failed ? 1 : 0;
}
