// ssq_fft.h -- the host FFT layer: one wrapper over a rocFFT plan (FftPlan: create / execute / destroy by hand, every
// rocFFT call checked) and one bounded per-stream cache of such plans (StreamPlanCache).
#pragma once
#include "ssq_common.h"
#include <rocfft/rocfft.h>
#include <map>
#include <tuple>

namespace ssq {

int fft_global_setup();

struct FftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    void* work = nullptr;
    size_t work_bytes = 0;

    // 1-D batched transform. kind: 0 = real->hermitian forward (out of place; `out_stride` between the bins of one
    // transform -- n_hops with out_dist 1 writes the spectra transposed), 1 = complex inverse in place, 2 = complex
    // forward in place, 3 = hermitian->real inverse (out of place, rocFFT's default layout: created without a plan
    // description, so scale and distances must be left alone).
    // `scale` multiplies the result (1/M for a normalised inverse).
    int create(int kind, int dtype, size_t length, size_t batch, double scale,
               size_t in_dist = 0, size_t out_dist = 0, size_t out_stride = 1);
    int execute(void* in, void* out, hipStream_t stream);
    void destroy();
};

// the forward and the inverse plan of a route that runs both (ssq_icwt2, ssq_trigdiff)
struct FftPlanPair {
    FftPlan fwd, inv;
    void destroy() { fwd.destroy(); inv.destroy(); }
};

// Plans (and their rocFFT work buffers) per (dtype, a, b, stream), at most 16: a 17th key waits for the device, destroys
// every entry and starts over. `V` has destroy(). The caller locks `mu` around `get` and keeps it until its transform
// is enqueued, so that two host threads cannot interleave set_stream / execute on one plan.
template <typename V>
struct StreamPlanCache {
    static constexpr size_t capacity = 16;
    std::mutex mu;
    std::map<std::tuple<int, int64_t, int64_t, hipStream_t>, V> plans;

    // *out = the entry of the key, made by `make(V&) -> status` where there is none; a value whose `make` fails is
    // destroyed and not inserted
    template <typename Make>
    int get(int dtype, int64_t a, int64_t b, hipStream_t stream, V** out, Make&& make) {
        const auto key = std::make_tuple(dtype, a, b, stream);
        auto it = plans.find(key);
        if (it == plans.end()) {
            if (plans.size() >= capacity) {
                (void)hipDeviceSynchronize();
                for (auto& kv : plans) kv.second.destroy();
                plans.clear();
            }
            V v;
            const int rc = make(v);
            if (rc) { v.destroy(); return rc; }
            it = plans.emplace(key, v).first;
        }
        *out = &it->second;
        return 0;
    }
};

}  // namespace ssq
