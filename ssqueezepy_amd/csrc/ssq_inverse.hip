// ssq_inverse.hip -- device side of the inverse transforms (C ABI: ssq_colsum, ssq_band_colsum[_batch], ssq_istft[_batch]
// and their adjoints ssq_colsum_adjoint, ssq_band_colsum_adjoint, ssq_istft_adjoint; the fused inverse-STFT kernels
// they launch are in ssq_stft.hip). The inverses of the reference are reductions over the
// scale / frequency axis of arrays that already live on the device:
//   icwt (one integral)  x[j] = sum_i Re(Wx[i,j]) / norm(scale_i)      _cwt.py:472-476
//   issq_cwt, issq_stft  x[j] = sum_i Re(Tx[i,j])  (optionally inside curve bands)
//                                                  _ssq_cwt.py:368-408, _ssq_stft.py:190-197
//   istft                irfft of every column, overlap-add with window^a, divided by
//                        the overlap-added window^(a+1)        _stft.py:238-256
//   adjoint of stft      scale + transpose, inverse real transform, overlap-add with the window, no norm
//                        (stft_adjoint_composed: the route of ssq_stft_adjoint for float64 / any n_fft)
// Sums run in the reference's order (ascending row, one accumulator per column, in the
// array's own precision), so the reductions are bit-identical to the NumPy results.
// Compiled with -ffp-contract=off.
#include "ssq_common.h"
#include "ssq_fft.h"
#include "ssq_stft.h"
#include <algorithm>
#include <mutex>

namespace ssq {

// out[b][j] = sum_i Re(Z[b][i][j]) (/ div[i]); one thread per column, rows in order
template <typename T, bool DIV>
__global__ __launch_bounds__(64) void colsum_kernel(const T* __restrict__ Z, const T* __restrict__ div,
                                                     T* __restrict__ out, int64_t na, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const T* z = Z + 2 * ((int64_t)blockIdx.y * na * n + j);
    T acc = T(0);
    // the additions are a dependent chain (fixed order); the loads are not: 16 rows in flight
    constexpr int UN = 16;
    int64_t i = 0;
    for (; i + UN <= na; i += UN) {
        T v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) v[u] = z[2 * (i + u) * n];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            T t = v[u];
            if (DIV) t = t / div[i + u];
            acc = acc + t;
        }
    }
    for (; i < na; ++i) {
        T v = z[2 * i * n];
        if (DIV) v = v / div[i];
        acc = acc + v;
    }
    out[(int64_t)blockIdx.y * n + j] = acc;
}

// blockIdx.y = k < K: rows lo[k][j] .. hi[k][j] of column j, accumulated in double (the
// reference builds the mask in complex128); blockIdx.y == K: the rows no band covers,
// accumulated in the data's precision (the reference zeroes them in a copy of Tx)
template <typename T>
__global__ __launch_bounds__(256) void band_colsum_kernel(const T* __restrict__ Z,
                                                          const int32_t* __restrict__ lo,
                                                          const int32_t* __restrict__ hi, int K,
                                                          double* __restrict__ out, int64_t na,
                                                          int64_t n, int64_t band_stride) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int k = (int)blockIdx.y;
    // blockIdx.z: the signal; its bands are the shared ones (band_stride 0) or its own
    const T* z = Z + 2 * ((int64_t)blockIdx.z * na * n + j);
    lo += (int64_t)blockIdx.z * band_stride; hi += (int64_t)blockIdx.z * band_stride;
    out += (int64_t)blockIdx.z * (K + 1) * n;
    if (k < K) {
        double acc = 0.0;
        const int64_t a = lo[(int64_t)k * n + j], b = hi[(int64_t)k * n + j];
        for (int64_t i = a; i <= b && i < na; ++i) acc = acc + (double)z[2 * i * n];
        out[(int64_t)k * n + j] = acc;
    } else {
        T acc = T(0);
        for (int64_t i = 0; i < na; ++i) {
            bool covered = false;
            for (int c = 0; c < K; ++c)
                covered |= (i >= lo[(int64_t)c * n + j]) & (i <= hi[(int64_t)c * n + j]);
            if (!covered) acc = acc + z[2 * i * n];
        }
        out[(int64_t)K * n + j] = (double)acc;
    }
}

// gZ[b][i][j] = (g[b][j] (/ div[i]), 0): the adjoint of colsum_kernel. One streaming pass: a work-item holds V columns'
// gradients and writes them to ROWS rows, 16 bytes a store (V = 2 complex64 / 1 complex128; V = 1 with 8-byte stores for
// complex64 rows of an odd length, whose starts are not all 16-byte aligned). Every element is written once.
constexpr int CSA_ROWS = 8;
template <typename T, bool DIV, int V>
__global__ __launch_bounds__(256) void colsum_adjoint_kernel(const T* __restrict__ g, const T* __restrict__ div,
                                                             T* __restrict__ gZ, int64_t na, int64_t n) {
    typedef T vec_t __attribute__((ext_vector_type(2 * V)));
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (j >= n) return;
    const int64_t b = blockIdx.z, i0 = (int64_t)blockIdx.y * CSA_ROWS;
    T gv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) gv[v] = g[b * n + j + v];              // (V == 2 only where n is even: j + 1 < n)
    T* o = gZ + 2 * ((b * na + i0) * n + j);
#pragma unroll
    for (int r = 0; r < CSA_ROWS; ++r) {
        if (i0 + r >= na) break;
        vec_t out;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            T t = gv[v];
            if (DIV) t = t / div[i0 + r];
            out[2 * v] = t; out[2 * v + 1] = T(0);
        }
        *reinterpret_cast<vec_t*>(o + 2 * r * n) = out;
    }
}

// gZ[b][i][j] = (sum over the bands k that hold row i, ascending, of g[b][k][j], or g[b][K][j] where none does; 0):
// the adjoint of band_colsum_kernel, summed in double and rounded once to T
template <typename T>
__global__ __launch_bounds__(256) void band_colsum_adjoint_kernel(const double* __restrict__ g,
                                                                  const int32_t* __restrict__ lo,
                                                                  const int32_t* __restrict__ hi, int K,
                                                                  T* __restrict__ gZ, int64_t na, int64_t n,
                                                                  int64_t band_stride) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t b = blockIdx.z, i0 = (int64_t)blockIdx.y * CSA_ROWS;
    lo += b * band_stride + j; hi += b * band_stride + j;
    g += b * (K + 1) * n + j;
    T* o = gZ + 2 * ((b * na + i0) * n + j);
    for (int r = 0; r < CSA_ROWS && i0 + r < na; ++r) {
        const int64_t i = i0 + r;
        double acc = 0.0;
        bool covered = false;
        for (int k = 0; k < K; ++k) {
            const bool in = (i >= lo[(int64_t)k * n]) & (i <= hi[(int64_t)k * n]);
            if (in) acc = acc + g[(int64_t)k * n];
            covered |= in;
        }
        if (!covered) acc = g[(int64_t)K * n];
        o[2 * r * n] = (T)acc; o[2 * r * n + 1] = T(0);
    }
}

// St[c][f] = Sx[f][c] (one contiguous half-spectrum per frame for the C2R transform);
// the imaginary parts of DC and, for even n_fft, Nyquist do not enter an inverse real FFT
template <typename T>
__global__ __launch_bounds__(256) void spec_transpose_kernel(const T* __restrict__ Sx, T* __restrict__ St,
                                                             int64_t rows, int64_t n_hops, int even) {
    const int64_t total = rows * n_hops;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = t % rows, c = t / rows;
        T re = Sx[2 * (f * n_hops + c)], im = Sx[2 * (f * n_hops + c) + 1];
        if (f == 0 || (even && f == rows - 1)) im = T(0);
        St[2 * t] = re; St[2 * t + 1] = im;
    }
}

// overlap-add of the (unnormalised) inverse real transforms, window modulation, trim
template <typename T>
__global__ __launch_bounds__(256) void istft_ola_kernel(const T* __restrict__ frames,
                                                        const T* __restrict__ win_a,
                                                        const T* __restrict__ win_a1, T* __restrict__ x,
                                                        int64_t n_fft, int64_t n_hops, int64_t hop,
                                                        int64_t N, int modulated, T inv_n, T tiny) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    const int64_t p = s + n_fft / 2;                    // index in the untrimmed signal
    const int64_t half = n_fft / 2;
    const int64_t max_hops = (N - 1) / hop + 1;         // frames the norm counts (len(wn) = N + n_fft - 1)
    int64_t i0 = p - n_fft + 1;
    i0 = i0 <= 0 ? 0 : (i0 + hop - 1) / hop;
    const int64_t i1 = p / hop;
    T acc = T(0);
    double wn = 0.0;
    for (int64_t i = i0; i <= i1; ++i) {
        const int64_t r = p - i * hop;
        if (i < max_hops) wn = wn + (double)win_a1[r];
        if (i < n_hops) {
            int64_t src = r;
            if (modulated) { src = r - half; if (src < 0) src += n_fft; }   // fftshift along the frame
            const T v = frames[i * n_fft + src] * inv_n;
            acc = acc + v * win_a[r];
        }
    }
    if (wn > (double)tiny) acc = (T)((double)acc / wn);
    x[s] = acc;
}

// S[k] = sum_a F[a][k] * psih[a][k] (rows in order): the double-integral iCWT summed in
// the frequency domain, so that one inverse transform serves all scales
template <typename T>
__global__ __launch_bounds__(256) void mulsum_rows_kernel(const T* __restrict__ F, const T* __restrict__ psih,
                                                          T* __restrict__ S, int64_t na, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    T re = T(0), im = T(0);
    for (int64_t a = 0; a < na; ++a) {
        const T p = psih[a * n + k];
        re = re + F[2 * (a * n + k)] * p;
        im = im + F[2 * (a * n + k) + 1] * p;
    }
    S[2 * k] = re; S[2 * k + 1] = im;
}

template <typename T>
__global__ __launch_bounds__(256) void real_part_kernel(const T* __restrict__ S, T* __restrict__ out, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = S[2 * k];
}

static StreamPlanCache<FftPlanPair> g_icwt2_plans;

template <typename T>
static int icwt2_t(int dtype, void* Wp, const void* psih, void* out, int64_t na, int64_t n,
                   hipStream_t stream) {
    // plans (and their rocFFT work buffers) are per stream; the lock is held until everything
    // is enqueued, so two host threads cannot interleave set_stream / execute on one plan
    FftPlanPair* pp = nullptr;
    std::lock_guard<std::mutex> lock(g_icwt2_plans.mu);
    int rc = g_icwt2_plans.get(dtype, na, n, stream, &pp, [&](FftPlanPair& pr) {
        const int r = pr.fwd.create(2, dtype, (size_t)n, (size_t)na, 1.0);
        return r ? r : pr.inv.create(1, dtype, (size_t)n, 1, 1.0 / (double)n);
    });
    if (rc) return rc;
    rc = pp->fwd.execute(Wp, nullptr, stream);                    // forward FFT of every row, in place
    if (rc) return rc;
    StreamScratch scratch(stream);
    T* S = nullptr;
    rc = scratch.alloc(&S, (size_t)n * 2 * sizeof(T));
    if (rc) return rc;
    dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL((mulsum_rows_kernel<T>), grid, dim3(256), 0, stream, (const T*)Wp, (const T*)psih, S, na, n);
    rc = (hipGetLastError() == hipSuccess) ? pp->inv.execute(S, nullptr, stream) : -3;
    if (!rc) {
        hipLaunchKernelGGL((real_part_kernel<T>), grid, dim3(256), 0, stream, (const T*)S, (T*)out, n);
        if (hipGetLastError() != hipSuccess) rc = -3;
    }
    if (rc == -3) set_error("icwt2 kernel launch failed");
    return rc;
}

// ------------------------------------------------------------------- trigdiff
// F[r][k] *= 1j * xi[k] * fs, formed as the reference's complex expression
// `A_freqdom * 1j * xi * fs` rounds it (utils/common.py:220): the rotation is exact, then one
// rounding per real factor
template <typename T>
__global__ __launch_bounds__(256) void mul_ixi_kernel(T* __restrict__ F, const T* __restrict__ xi, T fs,
                                                      int64_t rows, int64_t n) {
    const int64_t total = rows * n;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const T x = xi[q % n];
        const T re = F[2 * q], im = F[2 * q + 1];
        F[2 * q] = (-im * x) * fs;
        F[2 * q + 1] = (re * x) * fs;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void unpad_rows_kernel(const T* __restrict__ F, T* __restrict__ out,
                                                         int64_t rows, int64_t n_up, int64_t n1, int64_t N) {
    const int64_t total = rows * N;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t r = q / N, j = q - r * N;
        out[2 * q] = F[2 * (r * n_up + n1 + j)];
        out[2 * q + 1] = F[2 * (r * n_up + n1 + j) + 1];
    }
}

static StreamPlanCache<FftPlanPair> g_trig_plans;

template <typename T>
static int trigdiff_t(int dtype, void* Ap, const void* xi, double fs, void* out, int64_t rows,
                      int64_t n_up, int64_t n1, int64_t N, hipStream_t stream) {
    FftPlanPair* pp = nullptr;
    std::lock_guard<std::mutex> lock(g_trig_plans.mu);    // per-stream plans; held until enqueued
    int rc = g_trig_plans.get(dtype, rows, n_up, stream, &pp, [&](FftPlanPair& pr) {
        const int r = pr.fwd.create(2, dtype, (size_t)n_up, (size_t)rows, 1.0);
        return r ? r : pr.inv.create(1, dtype, (size_t)n_up, (size_t)rows, 1.0 / (double)n_up);
    });
    if (rc) return rc;
    rc = pp->fwd.execute(Ap, nullptr, stream);
    if (rc) return rc;
    const int64_t total = rows * n_up;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL((mul_ixi_kernel<T>), dim3(blocks), dim3(256), 0, stream, (T*)Ap, (const T*)xi, (T)fs,
                       rows, n_up);
    SSQ_LAUNCH_CHECK();
    rc = pp->inv.execute(Ap, nullptr, stream);
    if (rc) return rc;
    const unsigned blocks2 = (unsigned)std::min<int64_t>((rows * N + 255) / 256, 65536);
    hipLaunchKernelGGL((unpad_rows_kernel<T>), dim3(blocks2), dim3(256), 0, stream, (const T*)Ap, (T*)out, rows,
                       n_up, n1, N);
    SSQ_LAUNCH_CHECK();
    return 0;
}

// inverse real transforms of n_hops frames of n_fft samples: ssq_istft and the composed adjoint of the STFT
static StreamPlanCache<FftPlan> g_istft_plans;             // one work buffer per stream

// (the caller holds g_istft_plans.mu until the transform is enqueued)
static int istft_irfft(int dtype, int64_t n_fft, int64_t n_hops, void* St, void* frames, hipStream_t stream) {
    FftPlan* f = nullptr;
    const int rc = g_istft_plans.get(dtype, n_fft, n_hops, stream, &f, [&](FftPlan& p) {
        return p.create(3, dtype, (size_t)n_fft, (size_t)n_hops, 1.0);
    });
    return rc ? rc : f->execute(St, frames, stream);
}

template <typename T>
static int istft_t(int dtype, const void* Sx, const void* win_a, const void* win_a1, void* x,
                   int64_t n_fft, int64_t n_hops, int64_t hop, int64_t N, int modulated,
                   hipStream_t stream) {
    const int64_t rows = n_fft / 2 + 1;
    StreamScratch scratch(stream);
    T* St = nullptr; T* frames = nullptr;
    int rc = scratch.alloc(&St, (size_t)rows * n_hops * 2 * sizeof(T));
    if (!rc) rc = scratch.alloc(&frames, (size_t)(n_fft + 2) * n_hops * sizeof(T));
    if (rc) return rc;
    const int64_t total = rows * n_hops;
    unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL((spec_transpose_kernel<T>), dim3(g), dim3(256), 0, stream, (const T*)Sx, St, rows,
                       n_hops, (int)(n_fft % 2 == 0));
    SSQ_LAUNCH_CHECK();
    {
        std::lock_guard<std::mutex> lock(g_istft_plans.mu);
        rc = istft_irfft(dtype, n_fft, n_hops, St, frames, stream);
    }
    if (rc) return rc;
    const T tiny = sizeof(T) == 4 ? (T)1.17549435e-38f : (T)2.2250738585072014e-308;
    hipLaunchKernelGGL((istft_ola_kernel<T>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream,
                       (const T*)frames, (const T*)win_a, (const T*)win_a1, (T*)x, n_fft, n_hops,
                       hop, N, modulated, (T)(T(1) / (T)n_fft), tiny);
    if (hipGetLastError() != hipSuccess) { set_error("istft_ola launch failed"); return -3; }
    return 0;
}

// ---- batched inverse STFT and its backward ------------------------------------------------------------------
// wn[s] = the overlap-added win_a1 at the untrimmed position s + n_fft / 2, over the frames the reference's window
// norm counts, in double (the sum istft_ola_kernel forms per sample): once per call, not per signal
template <typename T>
__global__ __launch_bounds__(256) void istft_norm_kernel(const T* __restrict__ win_a1, double* __restrict__ wn,
                                                         int64_t n_fft, int64_t hop, int64_t N) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    const int64_t p = s + n_fft / 2, max_hops = (N - 1) / hop + 1;
    int64_t i0 = p - n_fft + 1;
    i0 = i0 <= 0 ? 0 : (i0 + hop - 1) / hop;
    const int64_t i1 = p / hop;
    double acc = 0.0;
    for (int64_t i = i0; i <= i1 && i < max_hops; ++i) acc = acc + (double)win_a1[p - i * hop];
    wn[s] = acc;
}

// win_t[r] = win_a[frame position of the transform's index r]: the rotation by n_fft / 2 of a modulated frame
template <typename T>
__global__ __launch_bounds__(256) void window_rotate_kernel(const T* __restrict__ win_a, T* __restrict__ win_t,
                                                            int64_t n_fft, int modulated) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_fft) return;
    win_t[r] = win_a[modulated ? (r + n_fft / 2) % n_fft : r];
}

// upad[b][p] = g[b][p - lead] / wn[p - lead] (g itself where the forward did not divide), 0 outside the N samples
template <typename T>
__global__ __launch_bounds__(256) void istft_u_kernel(const T* __restrict__ g, const double* __restrict__ wn,
                                                      T* __restrict__ upad, int64_t N, int64_t lead, int64_t ulen, T tiny) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ulen) return;
    const int64_t s = p - lead;
    T v = T(0);
    if (s >= 0 && s < N) {
        v = g[(int64_t)blockIdx.y * N + s];
        const double d = wn[s];
        if (d > (double)tiny) v = (T)((double)v / d);
    }
    upad[(int64_t)blockIdx.y * ulen + p] = v;
}

static bool istft_takes_fused(int dtype, int64_t n_fft, int64_t n_hops, int64_t hop, int64_t N) {
    const bool pow2 = n_fft >= 128 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0;
    // (SSQ_DEBUG_ISTFT_COMPOSED: the composed route on a shape the fused kernels take, for comparisons)
    return dtype == SSQ_F32 && pow2 && hop >= 1 && N >= 1 && n_hops == (N - 1) / hop + 1 && hop < ((int64_t)1 << 24)
        && N + n_fft < ((int64_t)1 << 30) && !getenv("SSQ_DEBUG_ISTFT_COMPOSED");
}

template <typename T>
static int istft_batch_t(int dtype, const void* Sx, const void* win_a, const void* win_a1, void* x, int64_t batch,
                         int64_t n_fft, int64_t n_hops, int64_t hop, int64_t N, int modulated, hipStream_t stream) {
    const int64_t rows = n_fft / 2 + 1;
    if (!istft_takes_fused(dtype, n_fft, n_hops, hop, N)) {
        int rc = 0;
        for (int64_t b = 0; b < batch && !rc; ++b)
            rc = istft_t<T>(dtype, (const T*)Sx + (size_t)b * rows * n_hops * 2, win_a, win_a1, (T*)x + (size_t)b * N,
                            n_fft, n_hops, hop, N, modulated, stream);
        return rc;
    }
    StreamScratch scratch(stream);
    double* wn = nullptr; T* win_t = nullptr;
    int rc = scratch.alloc(&wn, (size_t)N * sizeof(double));
    if (!rc) rc = scratch.alloc(&win_t, (size_t)n_fft * sizeof(T));
    if (rc) return rc;
    hipLaunchKernelGGL((istft_norm_kernel<T>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (const T*)win_a1,
                       wn, n_fft, hop, N);
    hipLaunchKernelGGL((window_rotate_kernel<T>), dim3((unsigned)((n_fft + 255) / 256)), dim3(256), 0, stream,
                       (const T*)win_a, win_t, n_fft, modulated);
    if (hipGetLastError() != hipSuccess) { set_error("istft norm / window launch failed"); rc = -3; }
    if (!rc) rc = istft_fused(Sx, win_t, wn, x, batch, n_fft, n_hops, hop, N, modulated, stream);
    return rc;
}

template <typename T>
static int istft_adjoint_t(int dtype, const void* g, const void* win_a, const void* win_a1, void* gSx, int64_t batch,
                           int64_t n_fft, int64_t n_hops, int64_t hop, int64_t N, int modulated, hipStream_t stream) {
    const bool fused = istft_takes_fused(dtype, n_fft, n_hops, hop, N);
    // fused: u (batch, N), the kernel extends it with zeros; composed: u between n_fft / 2 and the frames' end of zeros
    const int64_t lead = fused ? 0 : n_fft / 2, ulen = fused ? N : (n_hops - 1) * hop + n_fft;
    StreamScratch scratch(stream);
    double* wn = nullptr; T* win_t = nullptr; T* u = nullptr;
    int rc = scratch.alloc(&wn, (size_t)N * sizeof(double));
    if (!rc) rc = scratch.alloc(&win_t, (size_t)n_fft * sizeof(T));
    if (!rc) rc = scratch.alloc(&u, (size_t)batch * ulen * sizeof(T));
    if (rc) return rc;
    const T tiny = sizeof(T) == 4 ? (T)1.17549435e-38f : (T)2.2250738585072014e-308;
    hipLaunchKernelGGL((istft_norm_kernel<T>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (const T*)win_a1,
                       wn, n_fft, hop, N);
    hipLaunchKernelGGL((window_rotate_kernel<T>), dim3((unsigned)((n_fft + 255) / 256)), dim3(256), 0, stream,
                       (const T*)win_a, win_t, n_fft, modulated);
    hipLaunchKernelGGL((istft_u_kernel<T>), dim3((unsigned)((ulen + 255) / 256), (unsigned)batch), dim3(256), 0, stream,
                       (const T*)g, (const double*)wn, u, N, lead, ulen, tiny);
    if (hipGetLastError() != hipSuccess) { set_error("istft adjoint: norm / window / u launch failed"); rc = -3; }
    if (!rc) rc = fused ? istft_adjoint_fused(u, win_t, gSx, batch, n_fft, n_hops, hop, N, modulated, stream)
                        : istft_adjoint_composed(dtype, u, win_t, gSx, batch, n_fft, n_hops, hop, ulen, modulated, stream);
    return rc;
}

// ---- composed adjoint of the STFT (float64, and every n_fft the fused kernel does not take) ----------------
// St[c][f] = g[f][c], scaled so that rocFFT's inverse real transform -- which sums the Hermitian completion of
// what it is given -- returns the one-sided sum Re sum_{k <= n_fft/2} g[k] e^{+2 pi i k n / n_fft}: interior bins
// halved, DC and (even n_fft) Nyquist real
template <typename T>
__global__ __launch_bounds__(256) void adjoint_spec_transpose_kernel(const T* __restrict__ g, T* __restrict__ St,
                                                                     int64_t rows, int64_t n_hops, int even) {
    const int64_t total = rows * n_hops;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = t % rows, c = t / rows;
        const bool edge = f == 0 || (even && f == rows - 1);
        const T re = g[2 * (f * n_hops + c)], im = g[2 * (f * n_hops + c) + 1];
        St[2 * t] = edge ? re : re * T(0.5);
        St[2 * t + 1] = edge ? T(0) : im * T(0.5);
    }
}

// ypad[p] (+)= sum over the frames i that hold padded position p, ascending, of frames[i][r] * win[r], r the
// transform's index of the frame's sample p - i hop (the forward's rotation when modulated)
template <typename T>
__global__ __launch_bounds__(256) void adjoint_ola_kernel(const T* __restrict__ frames, const T* __restrict__ win,
                                                          T* __restrict__ ypad, int64_t n_fft, int64_t n_hops,
                                                          int64_t hop, int64_t padlen, int modulated, int accumulate) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= padlen) return;
    const int64_t s20 = (n_fft + 1) / 2, s21 = n_fft / 2;
    const int64_t i0 = p < n_fft ? 0 : (p - n_fft) / hop + 1;
    const int64_t i1 = p / hop < n_hops - 1 ? p / hop : n_hops - 1;
    T acc = accumulate ? ypad[p] : T(0);
    for (int64_t i = i0; i <= i1; ++i) {
        const int64_t m = p - i * hop;
        const int64_t r = !modulated ? m : (m >= s21 ? m - s21 : m + s20);
        acc = acc + frames[i * n_fft + r] * win[r];
    }
    ypad[p] = acc;
}

template <typename T>
static int stft_adjoint_composed_t(int dtype, const void* gSx, const void* gdSx, const void* window,
                                   const void* diff_window, void* ypad, int64_t batch, int64_t n_fft, int64_t n_hops,
                                   int64_t hop, int64_t padlen, int modulated, hipStream_t stream) {
    const int64_t rows = n_fft / 2 + 1, total = rows * n_hops;
    StreamScratch scratch(stream);
    T* St = nullptr; T* frames = nullptr;
    int rc = scratch.alloc(&St, (size_t)total * 2 * sizeof(T));
    if (!rc) rc = scratch.alloc(&frames, (size_t)(n_fft + 2) * n_hops * sizeof(T));
    if (rc) return rc;
    const unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    for (int64_t b = 0; b < batch && !rc; ++b) {
        int accumulate = 0;
        for (int side = 0; side < 2 && !rc; ++side) {
            const T* src = (const T*)(side ? gdSx : gSx);
            if (!src) continue;
            hipLaunchKernelGGL((adjoint_spec_transpose_kernel<T>), dim3(g), dim3(256), 0, stream,
                               src + (size_t)b * total * 2, St, rows, n_hops, (int)(n_fft % 2 == 0));
            if (hipGetLastError() != hipSuccess) { set_error("adjoint_spec_transpose launch failed"); rc = -3; break; }
            {
                std::lock_guard<std::mutex> lock(g_istft_plans.mu);
                rc = istft_irfft(dtype, n_fft, n_hops, St, frames, stream);
            }
            if (rc) break;
            hipLaunchKernelGGL((adjoint_ola_kernel<T>), dim3((unsigned)((padlen + 255) / 256)), dim3(256), 0, stream,
                               (const T*)frames, (const T*)(side ? diff_window : window),
                               (T*)ypad + (size_t)b * padlen, n_fft, n_hops, hop, padlen, modulated, accumulate);
            if (hipGetLastError() != hipSuccess) { set_error("adjoint_ola launch failed"); rc = -3; }
            accumulate = 1;
        }
    }
    return rc;
}

int stft_adjoint_composed(int dtype, const void* gSx, const void* gdSx, const void* window, const void* diff_window,
                          void* ypad, int64_t batch, int64_t n_fft, int64_t n_hops, int64_t hop, int64_t padlen,
                          int modulated, hipStream_t stream) {
    SSQ_REQUIRE(n_fft >= 2, "stft adjoint: n_fft %lld", (long long)n_fft);
    return dispatch_dtype(dtype, [&](auto t) {
        return stft_adjoint_composed_t<decltype(t)>(dtype, gSx, gdSx, window, diff_window, ypad, batch, n_fft, n_hops,
                                                    hop, padlen, modulated, stream);
    });
}

}  // namespace ssq

using namespace ssq;

extern "C" {

int ssq_colsum(int dtype, const void* Z, const void* divisor, void* out, int64_t batch, int64_t na,
               int64_t n, void* stream) {
    SSQ_REQUIRE(Z && out, "ssq_colsum: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(batch >= 1 && batch <= 65535 && na >= 1 && n >= 1, "colsum: bad shape (%lld, %lld, %lld)",
                (long long)batch, (long long)na, (long long)n);
    dim3 grid((unsigned)((n + 63) / 64), (unsigned)batch);
    hipStream_t s = as_stream(stream);
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
#define LAUNCH(DIV) hipLaunchKernelGGL((colsum_kernel<T, DIV>), grid, dim3(64), 0, s, (const T*)Z, \
                                       (const T*)divisor, (T*)out, na, n)
        if (divisor) LAUNCH(true); else LAUNCH(false);
#undef LAUNCH
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_band_colsum(int dtype, const void* Z, const int32_t* lo, const int32_t* hi, int64_t ncomp,
                    double* out, int64_t na, int64_t n, void* stream) {
    SSQ_REQUIRE(Z && lo && hi && out, "ssq_band_colsum: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(ncomp >= 1 && ncomp <= 65534 && na >= 1 && n >= 1, "band_colsum: bad shape");
    return ssq_band_colsum_batch(dtype, Z, lo, hi, 0, ncomp, out, 1, na, n, stream);
}

int ssq_band_colsum_batch(int dtype, const void* Z, const int32_t* lo, const int32_t* hi, int bands_per_signal,
                          int64_t ncomp, double* out, int64_t batch, int64_t na, int64_t n, void* stream) {
    SSQ_REQUIRE(Z && lo && hi && out, "ssq_band_colsum_batch: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(ncomp >= 1 && ncomp <= 65534 && na >= 1 && n >= 1 && batch >= 1 && batch <= 65535,
                "band_colsum: bad shape");
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)(ncomp + 1), (unsigned)batch);
    const int64_t stride = bands_per_signal ? ncomp * n : 0;
    hipStream_t s = as_stream(stream);
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((band_colsum_kernel<T>), grid, dim3(256), 0, s, (const T*)Z, lo, hi, (int)ncomp, out, na, n,
                           stride);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_band_colsum_adjoint(int dtype, const double* g, const int32_t* lo, const int32_t* hi, int bands_per_signal,
                            int64_t ncomp, void* gZ, int64_t batch, int64_t na, int64_t n, void* stream) {
    SSQ_REQUIRE(g && lo && hi && gZ, "ssq_band_colsum_adjoint: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(ncomp >= 1 && ncomp <= 65534 && na >= 1 && n >= 1 && batch >= 1 && batch <= 65535
                && (na + CSA_ROWS - 1) / CSA_ROWS <= 65535, "band_colsum_adjoint: bad shape");
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)((na + CSA_ROWS - 1) / CSA_ROWS), (unsigned)batch);
    const int64_t stride = bands_per_signal ? ncomp * n : 0;
    hipStream_t s = as_stream(stream);
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((band_colsum_adjoint_kernel<T>), grid, dim3(256), 0, s, g, lo, hi, (int)ncomp, (T*)gZ, na, n,
                           stride);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_colsum_adjoint(int dtype, const void* g, const void* divisor, void* gZ, int64_t batch, int64_t na,
                       int64_t n, void* stream) {
    SSQ_REQUIRE(g && gZ, "ssq_colsum_adjoint: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(batch >= 1 && batch <= 65535 && na >= 1 && n >= 1 && (na + CSA_ROWS - 1) / CSA_ROWS <= 65535,
                "colsum_adjoint: bad shape (%lld, %lld, %lld)", (long long)batch, (long long)na, (long long)n);
    hipStream_t s = as_stream(stream);
    // (16-byte stores need 16-byte aligned rows: complex64 rows of an even length in an aligned array)
    const bool v2 = dtype == SSQ_F32 && n % 2 == 0 && ((uintptr_t)gZ & 15) == 0;
    const int64_t cols = v2 ? n / 2 : n;
    dim3 grid((unsigned)((cols + 255) / 256), (unsigned)((na + CSA_ROWS - 1) / CSA_ROWS), (unsigned)batch);
#define LAUNCH(T, DIV, V) hipLaunchKernelGGL((colsum_adjoint_kernel<T, DIV, V>), grid, dim3(256), 0, s, (const T*)g, \
                                             (const T*)divisor, (T*)gZ, na, n)
    if (dtype == SSQ_F64) { if (divisor) LAUNCH(double, true, 1); else LAUNCH(double, false, 1); }
    else if (v2) { if (divisor) LAUNCH(float, true, 2); else LAUNCH(float, false, 2); }
    else { if (divisor) LAUNCH(float, true, 1); else LAUNCH(float, false, 1); }
#undef LAUNCH
    SSQ_LAUNCH_CHECK();
    return 0;
}

int ssq_icwt2(int dtype, void* Wp, const void* psih, void* out, int64_t na, int64_t n_up, void* stream) {
    SSQ_REQUIRE(Wp && psih && out, "ssq_icwt2: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(na >= 1 && n_up >= 2, "icwt2: bad shape (%lld, %lld)", (long long)na, (long long)n_up);
    return dispatch_dtype(dtype, [&](auto t) {
        return icwt2_t<decltype(t)>(dtype, Wp, psih, out, na, n_up, as_stream(stream));
    });
}

int ssq_trigdiff(int dtype, void* Ap, const void* xi, double fs, void* out, int64_t rows, int64_t n_up,
                 int64_t n1, int64_t N, void* stream) {
    SSQ_REQUIRE(Ap && xi && out, "ssq_trigdiff: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(rows >= 1 && n_up >= 2 && n1 >= 0 && N >= 1 && n1 + N <= n_up,
                "trigdiff: bad shape (%lld, %lld) / slice (%lld, %lld)", (long long)rows, (long long)n_up,
                (long long)n1, (long long)N);
    return dispatch_dtype(dtype, [&](auto t) {
        return trigdiff_t<decltype(t)>(dtype, Ap, xi, fs, out, rows, n_up, n1, N, as_stream(stream));
    });
}

int ssq_istft(int dtype, const void* Sx, const void* win_a, const void* win_a1, void* x, int64_t n_fft,
              int64_t n_hops, int64_t hop_len, int64_t N, int modulated, void* stream) {
    SSQ_REQUIRE(Sx && win_a && win_a1 && x, "ssq_istft: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(n_fft >= 2 && n_hops >= 1 && hop_len >= 1 && N >= 1, "istft: bad sizes");
    return dispatch_dtype(dtype, [&](auto t) {
        return istft_t<decltype(t)>(dtype, Sx, win_a, win_a1, x, n_fft, n_hops, hop_len, N, modulated, as_stream(stream));
    });
}

int ssq_istft_batch(int dtype, const void* Sx, const void* win_a, const void* win_a1, void* x, int64_t batch,
                    int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N, int modulated, void* stream) {
    SSQ_REQUIRE(Sx && win_a && win_a1 && x, "ssq_istft_batch: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(n_fft >= 2 && n_hops >= 1 && hop_len >= 1 && N >= 1, "istft: bad sizes");
    SSQ_REQUIRE(batch >= 1 && batch <= 65535, "istft: batch %lld outside [1, 65535]", (long long)batch);
    return dispatch_dtype(dtype, [&](auto t) {
        return istft_batch_t<decltype(t)>(dtype, Sx, win_a, win_a1, x, batch, n_fft, n_hops, hop_len, N, modulated,
                                          as_stream(stream));
    });
}

int ssq_istft_adjoint(int dtype, const void* g, const void* win_a, const void* win_a1, void* gSx, int64_t batch,
                      int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N, int modulated, void* stream) {
    SSQ_REQUIRE(g && win_a && win_a1 && gSx, "ssq_istft_adjoint: null pointer");
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "bad dtype %d", dtype);
    SSQ_REQUIRE(n_fft >= 2 && n_hops >= 1 && hop_len >= 1 && N >= 1, "istft adjoint: bad sizes");
    SSQ_REQUIRE(batch >= 1 && batch <= 65535, "istft adjoint: batch %lld outside [1, 65535]", (long long)batch);
    return dispatch_dtype(dtype, [&](auto t) {
        return istft_adjoint_t<decltype(t)>(dtype, g, win_a, win_a1, gSx, batch, n_fft, n_hops, hop_len, N, modulated,
                                            as_stream(stream));
    });
}

const char* ssq_istft_algo(int dtype, int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N) {
    return istft_takes_fused(dtype, n_fft, n_hops, hop_len, N) ? "fused" : "rocfft";
}

}  // extern "C"
