// ssq_common.h -- internal helpers shared by the translation units of libssq_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>
#include "../../include/ssq_hip.h"

// make the compiler treat a value as lane-dependent (keeps a load of a lane-independent
// address on the vector memory path)
#ifndef SSQ_OPAQUE_V
#define SSQ_OPAQUE_V(x) asm volatile("" : "+v"(x))
#endif
// ... and as a wave-uniform value the compiler may not fold or hoist (it stays in a scalar register)
// occupancy the compiler must plan a kernel's registers for (wavefronts per SIMD: min, max)
#ifndef SSQ_WAVES_PER_EU
#define SSQ_WAVES_PER_EU(lo, hi) __attribute__((amdgpu_waves_per_eu(lo, hi)))
#endif
#ifndef SSQ_OPAQUE_S
#define SSQ_OPAQUE_S(x) asm volatile("" : "+s"(x))
// nothing moves across this point in the instruction scheduler (bounds how far ahead an unrolled loop's loads are hoisted)
#define SSQ_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

#ifndef SSQ_LDS_ADD_F64
// LDS float64 add without a return value at byte offset `off` of the workgroup's LDS
#define SSQ_LDS_ADD_F64(base, off, val) asm volatile("ds_add_f64 %0, %1" :: "v"((unsigned)(size_t)(base) + (unsigned)(off)), "v"(val) : "memory")
// ... at an LDS byte address worked out by the caller (SSQ_LDS_ADDR of the array, once, + its offsets), plus a
// constant: the pointer-to-address conversion above costs a null test and two adds per use
#define SSQ_LDS_ADDR(ptr) ((unsigned)(size_t)(ptr))
#define SSQ_LDS_ADD_F64_AT(addr, o, val) asm volatile("ds_add_f64 %0, %1 offset:%2" :: "v"(addr), "v"(val), "n"(o) : "memory")
// every LDS operation of this wavefront done, then the workgroup's barrier -- without the wait for
// vector memory that __syncthreads() implies (the loads in flight belong to the next tile)
#define SSQ_WG_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// a table the kernel never writes, read with a wavefront-uniform index: the constant address space
// makes the compiler fetch it through the scalar cache (s_load) instead of the vector memory path
#define SSQ_CONST_PTR(T, p) reinterpret_cast<const __attribute__((address_space(4))) T*>(reinterpret_cast<uintptr_t>(p))
#endif

// Packed float32 multiply-add with one half of a register pair broadcast to both lanes of the
// packed operation (v_pk_fma_f32 op_sel): acc.xy += w.xy * s.x  /  acc.xy += w.xy * s.y, and the
// same for the multiply. hipcc materialises the broadcast with two v_mov per operand instead
// (34 of 131 instructions of the tile kernel's inner row), hence the explicit forms; and
// ds_bpermute_b32 with its immediate offset, which hipcc re-adds in a VGPR per use.
#ifndef SSQ_PK_DEFINED
typedef float ssq_f2 __attribute__((ext_vector_type(2)));
#define SSQ_PK_MUL_LO(d, w, s) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(d) : "v"(w), "v"(s))
#define SSQ_PK_MUL_HI(d, w, s) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(d) : "v"(w), "v"(s))
#define SSQ_PK_FMA_LO(acc, w, s) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(w), "v"(s))
#define SSQ_PK_FMA_HI(acc, w, s) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(w), "v"(s))
#define SSQ_BPERMUTE_OFF(d, addr, v, off) asm volatile("ds_bpermute_b32 %0, %1, %2 offset:%3" : "=v"(d) : "v"(addr), "v"(v), "n"(off))
// bitfield insert: d = (m & a) | (~m & b) in one instruction (the compiler spells the select out as four)
#define SSQ_BFI(d, m, a, b) asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(m), "v"(a), "v"(b))
// complex product d = a b of two (re, im) register pairs in two packed instructions:
//   t = (a.x b.x, a.x b.y);  d = (-a.y b.y + t.x, a.y b.x + t.y)
// (hipcc spells a complex product out as two multiplies and two multiply-adds, or as packed
// operations fed by v_mov shuffles).
// The s_nop is the wait state gfx950 requires between a transcendental instruction (v_sin_f32,
// v_cos_f32: twiddles) and a vector instruction that reads its result: the compiler inserts it for
// its own instructions and cannot see into this block -- without it the product read stale
// registers whenever the twiddle came straight out of v_sin / v_cos (caught by the GPU suite).
#define SSQ_CMUL_PK(d, a, b) do { ssq_f2 t_;                                                               \
    asm("s_nop 0\n\tv_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t_) : "v"(a), "v"(b));                  \
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"                       \
        : "=v"(d) : "v"(a), "v"(b), "v"(t_)); } while (0)
// eight taps in one block: A = sum_t w_t.x s_t, D = sum_t w_t.y s_t (s_t = a complex sample, w_t = a pair of real
// weights), each component the same chain of multiply-adds as SSQ_PK_MUL/FMA_LO/HI build. One asm statement
// because the compiler pads every pair of dependent packed instructions that sit in separate statements with an
// s_nop (it cannot see that the instruction between them is one); here each accumulator's instructions alternate
// with the other's, which is the one wait state the packed forwarding needs.
#define SSQ_TAPS8(A, D, w, s0, s1, s2, s3, s4, s5, s6, s7)                                                    \
    asm volatile("v_pk_mul_f32 %0, %2, %10 op_sel_hi:[0,1]\n\t"                                               \
                 "v_pk_mul_f32 %1, %2, %10 op_sel:[1,0] op_sel_hi:[1,1]\n\t"                                  \
                 "v_pk_fma_f32 %0, %3, %11, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %3, %11, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                          \
                 "v_pk_fma_f32 %0, %4, %12, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %4, %12, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                          \
                 "v_pk_fma_f32 %0, %5, %13, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %5, %13, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                          \
                 "v_pk_fma_f32 %0, %6, %14, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %6, %14, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                          \
                 "v_pk_fma_f32 %0, %7, %15, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %7, %15, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                          \
                 "v_pk_fma_f32 %0, %8, %16, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %8, %16, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                          \
                 "v_pk_fma_f32 %0, %9, %17, %0 op_sel_hi:[0,1,1]\n\t"                                         \
                 "v_pk_fma_f32 %1, %9, %17, %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]"                                \
                 : "=&v"(A), "=&v"(D)                                                                         \
                 : "v"((w)[0]), "v"((w)[1]), "v"((w)[2]), "v"((w)[3]), "v"((w)[4]), "v"((w)[5]), "v"((w)[6]),  \
                   "v"((w)[7]), "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "v"(s5), "v"(s6), "v"(s7))
// The same for TWO points that share their samples (neighbouring columns of one row, tile3_kernel): weights wa / wb,
// four accumulators taken in turn -- every instruction's operands are three instructions old.
#define SSQ_TAPS_T_(t, ta, tb, ts)                                                                            \
                 "v_pk_fma_f32 %0, %" #ta ", %" #ts ", %0 op_sel_hi:[0,1,1]\n\t"                               \
                 "v_pk_fma_f32 %1, %" #ta ", %" #ts ", %1 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"                \
                 "v_pk_fma_f32 %2, %" #tb ", %" #ts ", %2 op_sel_hi:[0,1,1]\n\t"                               \
                 "v_pk_fma_f32 %3, %" #tb ", %" #ts ", %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
#define SSQ_TAPS8X2(A0, D0, A1, D1, wa, wb, s0, s1, s2, s3, s4, s5, s6, s7)                                    \
    asm volatile("v_pk_mul_f32 %0, %4, %20 op_sel_hi:[0,1]\n\t"                                               \
                 "v_pk_mul_f32 %1, %4, %20 op_sel:[1,0] op_sel_hi:[1,1]\n\t"                                  \
                 "v_pk_mul_f32 %2, %12, %20 op_sel_hi:[0,1]\n\t"                                              \
                 "v_pk_mul_f32 %3, %12, %20 op_sel:[1,0] op_sel_hi:[1,1]\n\t"                                 \
                 SSQ_TAPS_T_(1, 5, 13, 21) SSQ_TAPS_T_(2, 6, 14, 22) SSQ_TAPS_T_(3, 7, 15, 23)                 \
                 SSQ_TAPS_T_(4, 8, 16, 24) SSQ_TAPS_T_(5, 9, 17, 25) SSQ_TAPS_T_(6, 10, 18, 26)                \
                 SSQ_TAPS_T_(7, 11, 19, 27)                                                                   \
                 : "=&v"(A0), "=&v"(D0), "=&v"(A1), "=&v"(D1)                                                 \
                 : "v"((wa)[0]), "v"((wa)[1]), "v"((wa)[2]), "v"((wa)[3]), "v"((wa)[4]), "v"((wa)[5]),        \
                   "v"((wa)[6]), "v"((wa)[7]), "v"((wb)[0]), "v"((wb)[1]), "v"((wb)[2]), "v"((wb)[3]),        \
                   "v"((wb)[4]), "v"((wb)[5]), "v"((wb)[6]), "v"((wb)[7]),                                    \
                   "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "v"(s5), "v"(s6), "v"(s7))
// flip a wave-uniform 0/1 and take the wavefront's issue priority from it (2 or 0): the compiler's form of
// the same costs two more scalar instructions per use
#define SSQ_PRIO_TOGGLE(p) asm volatile("s_xor_b32 %0, %0, 1\n\ts_cmp_eq_u32 %0, 0\n\ts_cbranch_scc1 1f\n\t"  \
                                        "s_setprio 2\n\ts_branch 2f\n1:\n\ts_setprio 0\n2:" : "+s"(p) :: "scc")
#define SSQ_LDS_WAIT() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define SSQ_LDS_WAITN(n) asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(n) : "memory")
#endif

namespace ssq {

void set_error(const char* fmt, ...);
// a switch of the environment set to 0 (SSQ_DEBUG_X=0 turns X off) / set to this word
static inline bool env_is_zero(const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; }
static inline bool env_equals(const char* name, const char* word) { const char* v = getenv(name); return v && !strcmp(v, word); }

#define SSQ_CHECK_HIP(expr)                                                        \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            ssq::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                           __FILE__, __LINE__);                                    \
            return -2;                                                             \
        }                                                                          \
    } while (0)

#define SSQ_REQUIRE(cond, ...)                                                     \
    do {                                                                           \
        if (!(cond)) {                                                             \
            ssq::set_error(__VA_ARGS__);                                           \
            return -1;                                                             \
        }                                                                          \
    } while (0)

#define SSQ_LAUNCH_CHECK()                                                         \
    do {                                                                           \
        hipError_t _e = hipGetLastError();                                         \
        if (_e != hipSuccess) {                                                    \
            ssq::set_error("kernel launch failed: %s (%s:%d)",                     \
                           hipGetErrorString(_e), __FILE__, __LINE__);             \
            return -3;                                                             \
        }                                                                          \
    } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The one place where a call's data type picks the instantiation: `f(float{})` or `f(double{})`, a generic lambda
// that takes the type from its argument (`using T = decltype(t)`); returns f's status. For sites whose two arms
// are the same text but for the type -- an arm that differs in more stays written out.
template <typename F>
static inline int dispatch_dtype(int dtype, F&& f) { return dtype == SSQ_F32 ? f(float{}) : f(double{}); }
// ... and where a run-time flag does: `f(std::true_type{})` or `f(std::false_type{})`. Both arms are instantiated, so a
// combination that must not exist (a float64 weight product for float64 data) is masked inside f:
// `constexpr bool C64 = decltype(c)::value && sizeof(T) == 4`.
template <typename F>
static inline int dispatch_bool(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
template <int N> using int_c = std::integral_constant<int, N>;

// Launch a kernel that takes `lds` bytes of dynamic LDS, up to the 160 KiB of a CU: raise the function's limit, launch,
// check. The attribute is set at every launch (it belongs to the function ON THE CURRENT DEVICE, a flag per
// instantiation would leave a second device of the process without it; the call costs well under a microsecond) and
// always to the full 160 KiB, as the tile kernels always had it. The sites that used to set the launch's own size
// could undercut each other -- thread A sets 100 KiB, thread B sets 50 KiB, A's launch is refused -- so the constant
// is a fix of those sites, not only a fold.
constexpr size_t LDS_CAP = 160 * 1024;
template <typename K, typename... Args>
static inline int launch_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    SSQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)LDS_CAP));
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    SSQ_LAUNCH_CHECK();
    return 0;
}

// grid of a streaming kernel over `total` items
static inline unsigned stream_grid(int64_t total, int block = 256) {
    int64_t g = (total + block - 1) / block;
    const int64_t cap = 256 * 8 * 4;   // 256 CUs x 8 blocks, grid-stride the rest
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- refusals that several entries state word for word (`name` opens the message)
static inline int check_dtype(int dtype) {
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "dtype must be SSQ_F32 or SSQ_F64 (got %d)", dtype);
    return 0;
}
// (32-bit point indices inside; five complex64 planes of 2^32 points would be 172 GB)
static inline int check_point_count(const char* name, int64_t batch, int64_t rows, int64_t n) {
    SSQ_REQUIRE(rows <= (int64_t)0xFFFFFFFFll / n && batch <= (int64_t)0xFFFFFFFFll / (rows * n),
                "%s: %lld x %lld x %lld points, at most 2^32 - 1", name, (long long)batch, (long long)rows, (long long)n);
    return 0;
}
static inline int check_gamma(const char* name, double gamma) {
    SSQ_REQUIRE(gamma >= 0.0, "%s: gamma must be >= 0 (got %g)", name, gamma);
    return 0;
}

// A small table on the current device, keyed by (device, uploaded bytes): uploaded once and kept -- a call that finds
// its table enqueues nothing (no allocation, no copy, nothing for the host to wait for), so it can be captured into a
// graph once its table exists. The eight most recent tables stay; an older one is freed with hipFree, which waits for
// the kernels that may still read it.
struct DeviceTableCache {
    struct Entry { int dev; std::vector<unsigned char> bytes; void* d; };
    std::mutex mu;
    std::vector<Entry> kept;
    template <typename P>
    int get(const P* host, size_t count, const P** out) {
        const size_t bytes = count * sizeof(P);
        int dev = 0;
        SSQ_CHECK_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lock(mu);
        for (const Entry& t : kept)
            if (t.dev == dev && t.bytes.size() == bytes && memcmp(t.bytes.data(), host, bytes) == 0) {
                *out = static_cast<const P*>(t.d);
                return 0;
            }
        if (kept.size() >= 8) {
            (void)hipFree(kept.front().d);
            kept.erase(kept.begin());
        }
        void* d = nullptr;
        SSQ_CHECK_HIP(hipMalloc(&d, bytes));
        hipError_t e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); SSQ_CHECK_HIP(e); }
        const unsigned char* b = reinterpret_cast<const unsigned char*>(host);
        kept.push_back(Entry{dev, std::vector<unsigned char>(b, b + bytes), d});
        *out = static_cast<const P*>(d);
        return 0;
    }
};

// Stream-ordered temporaries of one host function: `alloc` is hipMallocAsync on the guard's stream, the
// destructor hipFreeAsync on the same stream for everything handed out, in that order -- at every return.
struct StreamScratch {
    hipStream_t stream;
    std::vector<void*> held;
    explicit StreamScratch(hipStream_t s) : stream(s) {}
    StreamScratch(const StreamScratch&) = delete;
    StreamScratch& operator=(const StreamScratch&) = delete;
    template <typename P>
    int alloc(P** ptr, size_t bytes) {
        void* p = nullptr;
        *ptr = nullptr;
        SSQ_CHECK_HIP(hipMallocAsync(&p, bytes, stream));
        held.push_back(p);
        *ptr = static_cast<P*>(p);
        return 0;
    }
    ~StreamScratch() { for (void* p : held) (void)hipFreeAsync(p, stream); }
};

// The device allocations of one plan object (hipMalloc; StreamScratch above is the stream-ordered kind for one call's
// temporaries): `alloc` / `upload` hand memory out -- 1 byte where 0 are asked for, so that every table has an
// address --, `bytes` is what was asked for so far, `release` frees it all. A setup that must complete or leave the
// plan as it found it notes `count()` first and, on failure, gives `release` that number: what came after it is freed.
struct DeviceArena {
    struct Held { void* p; size_t bytes; };
    std::vector<Held> held;
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    template <typename P>
    int alloc(P** ptr, size_t bytes) {
        void* p = nullptr;
        *ptr = nullptr;
        SSQ_CHECK_HIP(hipMalloc(&p, bytes ? bytes : 1));
        held.push_back(Held{p, bytes});
        *ptr = static_cast<P*>(p);
        return 0;
    }
    template <typename P>
    int upload(P** ptr, const void* host, size_t bytes) {
        const int rc = alloc(ptr, bytes);
        if (rc) return rc;
        if (bytes) SSQ_CHECK_HIP(hipMemcpy(*ptr, host, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    size_t count() const { return held.size(); }
    int64_t bytes() const {
        int64_t total = 0;
        for (const Held& h : held) total += (int64_t)h.bytes;
        return total;
    }
    void release(size_t keep = 0) {
        while (held.size() > keep) { (void)hipFree(held.back().p); held.pop_back(); }
    }
};

// A plan under construction, from `new` to the line that hands it over (`release`): destroyed at every other return.
template <typename P> using PlanGuard = std::unique_ptr<P, void (*)(P*)>;

// A cached plan owns device workspaces that every execute reuses. Executes are asynchronous
// and torch's side streams do not synchronise with each other, so two executes of one plan on
// different streams (or from two host threads) would overwrite each other's workspace. `enter`
// makes the new stream wait for the plan's previous execute (one event, recorded by `leave`);
// the mutex serialises the host side for the duration of the enqueue.
struct PlanOrder {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    int enter(hipStream_t s) {
        mu.lock();
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; return 0; }
        if (used && last != s) (void)hipStreamWaitEvent(s, ev, 0);
        return 0;
    }
    void leave(hipStream_t s) {
        if (ev) { (void)hipEventRecord(ev, s); used = true; last = s; }
        mu.unlock();
    }
    void destroy() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
};
// per-row reassignment weights on the device: a new buffer for every new content (an execute
// already enqueued keeps reading the one it was given); all freed with the plan
struct WeightVersions {
    std::vector<void*> bufs;
    int upload(void** current, const void* host, size_t bytes) {
        void* p = nullptr;
        if (bufs.size() >= 32) {                 // bounded: recycle after draining the device
            (void)hipDeviceSynchronize();
            for (size_t i = 0; i + 1 < bufs.size(); ++i) (void)hipFree(bufs[i]);
            void* keep = bufs.back(); bufs.clear(); bufs.push_back(keep);
        }
        SSQ_CHECK_HIP(hipMalloc(&p, bytes ? bytes : 1));
        SSQ_CHECK_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
        bufs.push_back(p);
        *current = p;
        return 0;
    }
    void destroy() { for (void* p : bufs) (void)hipFree(p); bufs.clear(); }
};

// The signal-extension rule, for pad_kernel on the device and for its transpose below on the host:
// t in [-n1, n + n2); returns the source index in [0, n) or -1 for zero fill
__host__ __device__ static inline int64_t pad_source(int64_t t, int64_t n, int padtype) {
    if (t >= 0 && t < n) return t;
    switch (padtype) {
        case SSQ_PAD_REFLECT: {
            if (n == 1) return 0;
            int64_t period = 2 * (n - 1);
            int64_t m = t % period; if (m < 0) m += period;
            return m < n ? m : period - m;
        }
        case SSQ_PAD_SYMMETRIC: {
            int64_t period = 2 * n;
            int64_t m = t % period; if (m < 0) m += period;
            return m < n ? m : period - 1 - m;
        }
        case SSQ_PAD_REPLICATE: return t < 0 ? 0 : n - 1;
        case SSQ_PAD_WRAP: { int64_t m = t % n; if (m < 0) m += n; return m; }
        default: return -1;
    }
}

// The transpose of a signal extension, for the adjoints (ssq_stft_adjoint, ssq_cwt_adjoint): the padded positions
// p in [0, m) that copy signal sample j -- position p reads sample p - n1 through pad_source --, per j,
// ascending: `idx[off[j] .. off[j + 1])`. Zero padding has no source and is left out. m < 2^31.
static inline void inverse_pad_table(int64_t n, int64_t m, int64_t n1, int padtype, std::vector<int32_t>& off,
                                     std::vector<int32_t>& idx) {
    off.assign((size_t)n + 1, 0);
    for (int64_t p = 0; p < m; ++p) { const int64_t j = pad_source(p - n1, n, padtype); if (j >= 0) ++off[(size_t)j + 1]; }
    for (int64_t j = 0; j < n; ++j) off[(size_t)j + 1] += off[(size_t)j];
    idx.assign((size_t)off[(size_t)n], 0);
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (int64_t p = 0; p < m; ++p) { const int64_t j = pad_source(p - n1, n, padtype); if (j >= 0) idx[(size_t)fill[(size_t)j]++] = (int32_t)p; }
}

template <typename T> struct cplx { T re, im; };

// reassignment parameters as the kernels consume them
struct SsqParams {
    double p[5];      // see SSQ_GRID_* in ssq_hip.h
    double gamma;
    int    grid;
    int    flipud;
    int    cst_f64;
    int    cst_uniform;   // all per-row weights equal (scalar `const`): kernels read one value
    // float32 screening of the bin map (ssq_point_math.inl: bin_screen_f32): the bin
    // is first estimated in float32; only points whose estimate lies within `guard`
    // bins of a rounding boundary are re-evaluated with the exact double sequence.
    float  pf[5];     // p[] rounded to float (pf[1], pf[2], pf[3] hold reciprocals)
    float  guard;     // >= 0.25 disables screening
};

// fill the float32 screening constants from p[]/grid
static inline void finalize_params(SsqParams& sp) {
    // abs. error budget of the float32 chain (log2 w - vlmin): v_log_f32 is good to 1 ulp
    // (<= 1e-6 for |log2 w| < 16), float(vlmin) and the subtraction round by <= 5e-7
    // each -> 2e-6; budgeted 2.5x. Relative terms are added per point.
    const double slack = 5e-6;
    double g;
    if (sp.grid == SSQ_GRID_LIN) {
        sp.pf[0] = (float)sp.p[0]; sp.pf[1] = (float)(1.0 / sp.p[1]);
        g = 1e-6;                         // relative part is added per point
    } else if (sp.grid == SSQ_GRID_LOG) {
        sp.pf[0] = (float)sp.p[0]; sp.pf[1] = (float)(1.0 / sp.p[1]);
        g = slack / sp.p[1];
    } else {
        sp.pf[0] = (float)sp.p[0]; sp.pf[1] = (float)sp.p[1];
        sp.pf[2] = (float)(1.0 / sp.p[2]); sp.pf[3] = (float)(1.0 / sp.p[3]);
        sp.pf[4] = (float)sp.p[4];
        double dmin = sp.p[2] < sp.p[3] ? sp.p[2] : sp.p[3];
        g = slack / dmin;
    }
    if (!(g < 0.25)) g = 1.0;
    sp.guard = (float)g;
}

// the parameters of a C-ABI call; `name`, where given, opens the refusals' messages
static inline int fill_params(SsqParams& sp, int grid, const double* params, int flipud, double gamma, int cst_f64,
                              const char* name = nullptr) {
    const bool known = grid >= SSQ_GRID_LOG && grid <= SSQ_GRID_LIN;
    if (name) SSQ_REQUIRE(known, "%s: unknown grid kind %d", name, grid);
    SSQ_REQUIRE(known, "unknown grid kind %d", grid);
    SSQ_REQUIRE(params, "grid params must not be null");
    for (int t = 0; t < 5; ++t) sp.p[t] = params[t];
    sp.grid = grid; sp.flipud = flipud ? 1 : 0; sp.gamma = gamma; sp.cst_f64 = cst_f64 ? 1 : 0;
    sp.cst_uniform = 0;                   // weights are a device array here: not inspected
    finalize_params(sp);
    return 0;
}

// ssq_cwt_plan_set_ssq / ssq_stft_plan_set_ssq: the parameters of a plan of `dtype` from the call's arguments, and a new
// version of its `rows` per-row weights, which come from the host here (float64 where cst_f64 or the plan is float64;
// a float64 plan's kernels read them as their own type, so cst_f64 is not set for one). Notes when the weights are one
// scalar repeated, and the first of them. The caller holds the plan's PlanOrder::mu: kernels receive SsqParams by value
// at launch, so an execute already enqueued keeps its own, and the lock orders this update against an execute that
// another host thread is enqueuing.
static inline int set_ssq_params(SsqParams& sp, WeightVersions& weights, void** cst_dev, float* cst0, int dtype,
                                 int64_t rows, int grid, const double* params, const void* cst, int cst_f64, int flipud,
                                 double gamma) {
    const int rc = fill_params(sp, grid, params, flipud, gamma, cst_f64 && dtype == SSQ_F32);
    if (rc) return rc;
    const bool wide = cst_f64 || dtype == SSQ_F64;
    bool uni = true;
    for (int64_t i = 1; i < rows && uni; ++i)
        uni = wide ? ((const double*)cst)[i] == ((const double*)cst)[0] : ((const float*)cst)[i] == ((const float*)cst)[0];
    sp.cst_uniform = uni ? 1 : 0;
    *cst0 = wide ? (float)((const double*)cst)[0] : ((const float*)cst)[0];
    return weights.upload(cst_dev, cst, (size_t)rows * (wide ? 8 : 4));
}

// ---- launchers implemented in ssq_kernels.hip, used by the plans --------------
// SSQ_TILE_ORDER=ordered: reassignment sums in the CPU path's order (bit-exact kernels)
bool reassign_ordered();
// bin source for the accumulate kernel
enum BinSrc { BIN_FROM_DWX = 0, BIN_FROM_W = 1, BIN_FROM_KIDX = 2 };

// Tx <- accumulate(Wx, src) ; src is dWx (complex), w (real) or kidx (uint16)
int launch_accumulate(int dtype, int binsrc, const void* Wx, const void* src,
                      const void* Sfs, void* Tx, const void* cst,
                      const SsqParams& sp, int64_t batch, int64_t na, int64_t n,
                      int32_t* kmap, hipStream_t stream);

}  // namespace ssq
