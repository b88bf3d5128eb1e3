// host_fft_check.cpp -- the plan cache (csrc/ssq_fft.h: StreamPlanCache) and the scratch guard (csrc/ssq_common.h:
// StreamScratch) driven on the host, against the emulator's headers (tests/emu/hip, tests/emu/rocfft), with the
// runtime calls they make counted here. A program of its own: tests/test_host_fft_layer.py builds it with
// -fsanitize=address,undefined and runs it. TEST INFRASTRUCTURE ONLY.
#include "hip/hip_runtime.h"
#include <set>

static std::set<void*> g_live;                 // what counted_malloc_async handed out and nobody freed yet
static int g_mallocs = 0, g_frees = 0, g_syncs = 0, g_bad_frees = 0, g_fail_malloc_at = 0;
static hipStream_t g_stream = (hipStream_t)0x51;

static hipError_t counted_malloc_async(void** p, size_t n, hipStream_t s) {
    if (s != g_stream) return 3;
    if (++g_mallocs == g_fail_malloc_at) { *p = nullptr; return 2; }
    *p = malloc(n ? n : 1);
    g_live.insert(*p);
    return hipSuccess;
}
static hipError_t counted_free_async(void* p, hipStream_t s) {
    if (s != g_stream || !g_live.erase(p)) { ++g_bad_frees; return 1; }
    free(p);
    ++g_frees;
    return hipSuccess;
}
static hipError_t counted_device_synchronize() { ++g_syncs; return hipSuccess; }
#define hipMallocAsync counted_malloc_async
#define hipFreeAsync counted_free_async
#define hipDeviceSynchronize counted_device_synchronize

#include "ssq_fft.h"

namespace ssq {
void set_error(const char*, ...) {}
}

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

// ---- the cache
static int g_made = 0, g_destroyed = 0;
struct Counted {                                // two halves, like a pair of plans
    bool first = false, second = false;
    void destroy() {
        if (first) { ++g_destroyed; first = false; }
        if (second) { ++g_destroyed; second = false; }
    }
};
static int make_both(Counted& c) { c.first = c.second = true; g_made += 2; return 0; }
static int make_half_then_fail(Counted& c) { c.first = true; ++g_made; return -4; }

static void check_cache() {
    ssq::StreamPlanCache<Counted> cache;
    std::lock_guard<std::mutex> lock(cache.mu);
    Counted* at[17] = {nullptr};
    for (int k = 0; k < 16; ++k) CHECK(cache.get(SSQ_F64, 16, 10 + k, g_stream, &at[k], make_both) == 0);
    CHECK(cache.plans.size() == 16 && g_made == 32 && g_destroyed == 0 && g_syncs == 0);     // 16 keys stay resident
    // a resident key: the same object, `make` not called
    for (int k = 0; k < 16; ++k) {
        Counted* again = nullptr;
        CHECK(cache.get(SSQ_F64, 16, 10 + k, g_stream, &again, make_both) == 0 && again == at[k]);
    }
    CHECK(g_made == 32 && g_destroyed == 0 && g_syncs == 0);
    // every part of the key tells entries apart; a failing make leaves no entry and destroys what it half built --
    // here at a full cache, which it empties first, as the 17th key does
    Counted* none = nullptr;
    CHECK(cache.get(SSQ_F64, 16, 26, g_stream, &none, make_half_then_fail) == -4 && none == nullptr);
    CHECK(g_syncs == 1 && g_destroyed == 32 + 1 && g_made == 33 && cache.plans.empty());
    g_made = g_destroyed = g_syncs = 0;
    for (int k = 0; k < 16; ++k) CHECK(cache.get(k % 2 ? SSQ_F32 : SSQ_F64, 16 + k / 8, 10 + k % 4, k % 8 < 4 ? g_stream : nullptr,
                                                 &at[k], make_both) == 0);
    CHECK(cache.plans.size() == 16 && g_made == 32);
    // the 17th key: one wait for the device, exactly the 16 entries destroyed, the new one alone in the cache
    CHECK(cache.get(SSQ_F64, 16, 99, g_stream, &at[16], make_both) == 0);
    CHECK(g_syncs == 1 && g_destroyed == 32 && g_made == 34 && cache.plans.size() == 1 && at[16]->first && at[16]->second);
    // a failing make at a cache with room: the entries stay, nothing is inserted
    CHECK(cache.get(SSQ_F64, 16, 100, g_stream, &none, make_half_then_fail) == -4);
    CHECK(g_syncs == 1 && g_destroyed == 33 && cache.plans.size() == 1);
    for (auto& kv : cache.plans) kv.second.destroy();
    CHECK(g_destroyed == 35);
}

// ---- the guard
static int two_allocations(bool leave_between, float** a_out) {
    ssq::StreamScratch scratch(g_stream);
    float* a = nullptr; double* b = nullptr;
    int rc = scratch.alloc(&a, 64 * sizeof(float));
    if (rc) return rc;
    a[63] = 1.f;                                            // (the memory is the caller's until the guard goes)
    *a_out = a;
    if (leave_between) return -3;                           // what SSQ_LAUNCH_CHECK does after a failed launch
    rc = scratch.alloc(&b, 32 * sizeof(double));
    if (rc) return rc;
    b[31] = 1.;
    CHECK(g_live.size() == 2 && g_frees == 0);              // nothing is freed before the function returns
    return 0;
}

static void check_guard() {
    float* a = nullptr;
    CHECK(two_allocations(false, &a) == 0 && g_mallocs == 2 && g_frees == 2 && g_live.empty());
    g_mallocs = g_frees = 0;
    CHECK(two_allocations(true, &a) == -3 && g_mallocs == 1 && g_frees == 1 && g_live.empty());    // early return
    g_mallocs = g_frees = 0;
    g_fail_malloc_at = 2;                                   // the second allocation fails: the first is freed
    CHECK(two_allocations(false, &a) == -2 && g_mallocs == 2 && g_frees == 1 && g_live.empty());
    g_fail_malloc_at = 0;
    CHECK(g_bad_frees == 0);
    { ssq::StreamScratch unused(g_stream); }
    CHECK(g_frees == 1 && g_bad_frees == 0);
}

static void check_dispatch() {
    CHECK(ssq::dispatch_dtype(SSQ_F32, [](auto t) { return (int)sizeof(t); }) == 4);
    CHECK(ssq::dispatch_dtype(SSQ_F64, [](auto t) { return (int)sizeof(t); }) == 8);
}

int main() {
    check_cache();
    check_guard();
    check_dispatch();
    printf(g_failed ? "FAIL\n" : "PASS\n");
    return g_failed ? 1 : 0;
}
