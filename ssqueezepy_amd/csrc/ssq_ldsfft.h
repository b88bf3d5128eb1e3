// ssq_ldsfft.h -- complex FFT building blocks shared by the fused kernels, for float and
// double: in-register radix-4/8/16 butterflies and `lds_ifft`, a Stockham inverse FFT of G
// columns of L points through LDS, 16 points per thread (float: 4096 complex points per
// 256-thread workgroup; double: 2048 points per 128-thread workgroup -- both 32 KiB of LDS).
// A transform's shape is its length: `FftShape<L, R>` holds the columns per workgroup and the two or
// three radices that go with L, `fft_switch` / `fft_dispatch` turn a run-time length into that tag.
// Used by the CWT block / four-step kernels (ssq_cwt_blocks.hip, ssq_tile_fft.hip) and the fused STFT
// kernels (ssq_stft.hip). Include inside a .hip translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include "ssq_common.h"
#include <cmath>
#include <type_traits>
#include <vector>

namespace ssq {

template <typename R> struct cx { R x, y; };
using c32 = cx<float>;
using c64 = cx<double>;

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename R> __device__ __forceinline__ cx<R> cmul(cx<R> a, cx<R> b) {
    return {fma_(a.x, b.x, -(a.y * b.y)), fma_(a.x, b.y, a.y * b.x)};
}
// the same product for operands that live in registers (twiddles from tables, data): float32 in two
// packed instructions (SSQ_CMUL_PK; rounds the a.x products first, where `cmul` rounds the a.y ones)
__device__ __forceinline__ cx<float> cmul_v(cx<float> a, cx<float> b) {
    ssq_f2 av, bv, dv;
    av.x = a.x; av.y = a.y; bv.x = b.x; bv.y = b.y;
    SSQ_CMUL_PK(dv, av, bv);
    return {dv.x, dv.y};
}
__device__ __forceinline__ cx<double> cmul_v(cx<double> a, cx<double> b) { return cmul(a, b); }
template <typename R> __device__ __forceinline__ cx<R> cadd(cx<R> a, cx<R> b) { return {a.x + b.x, a.y + b.y}; }
template <typename R> __device__ __forceinline__ cx<R> csub(cx<R> a, cx<R> b) { return {a.x - b.x, a.y - b.y}; }
// multiply by +i (inverse-transform rotation)
template <typename R> __device__ __forceinline__ cx<R> mul_i(cx<R> a) { return {-a.y, a.x}; }

// in-place inverse DFTs: V[k] = sum_t v[t] e^{+2 pi i t k / R}
template <typename R> __device__ __forceinline__ void dft2(cx<R>& a, cx<R>& b) { cx<R> t = a; a = cadd(t, b); b = csub(t, b); }

template <typename R>
__device__ __forceinline__ void dft4(cx<R>& v0, cx<R>& v1, cx<R>& v2, cx<R>& v3) {
    cx<R> a = cadd(v0, v2), b = csub(v0, v2), c = cadd(v1, v3), d = mul_i(csub(v1, v3));
    v0 = cadd(a, c); v1 = cadd(b, d); v2 = csub(a, c); v3 = csub(b, d);
}

template <int R> struct Dft;
template <> struct Dft<4> {
    template <typename R> static __device__ __forceinline__ void run(cx<R> (&v)[4]) { dft4(v[0], v[1], v[2], v[3]); }
};
template <> struct Dft<8> {
    template <typename R> static __device__ __forceinline__ void run(cx<R> (&v)[8]) {
        // 8 = 2 x 4, decimation in time: even/odd 4-point DFTs, twiddle W8^k
        cx<R> e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
        dft4(e[0], e[1], e[2], e[3]);
        dft4(o[0], o[1], o[2], o[3]);
        const R h = (R)0.70710678118654752440;
        o[1] = {h * (o[1].x - o[1].y), h * (o[1].x + o[1].y)};     // * e^{+i pi/4}
        o[2] = mul_i(o[2]);                                        // * e^{+i pi/2}
        o[3] = {-h * (o[3].x + o[3].y), h * (o[3].x - o[3].y)};    // * e^{+i 3pi/4}
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = cadd(e[k], o[k]); v[k + 4] = csub(e[k], o[k]); }
    }
};
template <> struct Dft<16> {
    template <typename R> static __device__ __forceinline__ void run(cx<R> (&v)[16]) {
        // 16 = 4 x 4: t = t1 + 4 t2, k = 4 k1 + k2 ... columns t1, DFT over t2, twiddle, DFT over t1
        const R c1 = (R)0.92387953251128675613, s1 = (R)0.38268343236508977173;   // cos/sin(pi/8)
        const R h = (R)0.70710678118654752440;
        cx<R> a[4][4];
#pragma unroll
        for (int t1 = 0; t1 < 4; ++t1) {
            a[t1][0] = v[t1]; a[t1][1] = v[t1 + 4]; a[t1][2] = v[t1 + 8]; a[t1][3] = v[t1 + 12];
            dft4(a[t1][0], a[t1][1], a[t1][2], a[t1][3]);      // index k2
        }
        // twiddle W16^{t1*k2} = e^{+2 pi i t1 k2 / 16}
        const cx<R> w[10] = {{1, 0}, {c1, s1}, {h, h}, {s1, c1}, {0, 1}, {-s1, c1}, {-h, h}, {-c1, s1},
                           {-1, 0}, {-c1, -s1}};
#pragma unroll
        for (int t1 = 1; t1 < 4; ++t1)
#pragma unroll
            for (int k2 = 1; k2 < 4; ++k2) a[t1][k2] = cmul(a[t1][k2], w[t1 * k2]);
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            cx<R> b0 = a[0][k2], b1 = a[1][k2], b2 = a[2][k2], b3 = a[3][k2];
            dft4(b0, b1, b2, b3);                               // index k1
            v[k2] = b0; v[k2 + 4] = b1; v[k2 + 8] = b2; v[k2 + 12] = b3;
        }
    }
};

constexpr int PPT = 16;            // points per thread
template <typename R> struct FftGeom {
    static constexpr int NT = sizeof(R) == 4 ? 256 : 128;   // threads per workgroup
    static constexpr int D = NT * PPT;                      // complex points per workgroup
};
constexpr int D_POINTS = FftGeom<float>::D;     // float32 kernels: 4096 points,
constexpr int NT = FftGeom<float>::NT;          //                  256 threads

// ---- the shapes lds_ifft runs: 64 .. 4096 points, and everything but the length follows from it
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
// G: columns per workgroup; R1, R2, R3: the Stockham radices in pass order (R3 = 1: two passes); RL: the last one.
// Two passes up to 256 points, three from 512 on; radix 16 for as many passes as the length allows, the first ones.
template <int L, typename R = float> struct FftShape {
    static_assert(L >= 64 && L <= 4096 && (L & (L - 1)) == 0, "FftShape: a power of two in [64, 4096]");
    static constexpr int LOG2L = ilog2(L);
    static constexpr int G = FftGeom<R>::D / L;
    static constexpr int NPASS = L <= 256 ? 2 : 3, N16 = LOG2L - 3 * NPASS;
    static constexpr int R1 = N16 >= 1 ? 16 : 8, R2 = N16 >= 2 ? 16 : 8, R3 = NPASS < 3 ? 1 : N16 >= 3 ? 16 : 8;
    static constexpr int RL = (R3 > 1) ? R3 : R2;
    static_assert(R1 * R2 * R3 == L && G >= 1, "FftShape: the radices make up the length");
};
// the derivation against the tuples the kernels were written out with
template <int L, int G, int R1, int R2, int R3, typename R = float, typename S = FftShape<L, R>>
constexpr bool fft_shape_is() { return S::G == G && S::R1 == R1 && S::R2 == R2 && S::R3 == R3; }
static_assert(fft_shape_is<64, 64, 8, 8, 1>() && fft_shape_is<128, 32, 16, 8, 1>() && fft_shape_is<256, 16, 16, 16, 1>() &&
              fft_shape_is<512, 8, 8, 8, 8>() && fft_shape_is<1024, 4, 16, 8, 8>() && fft_shape_is<2048, 2, 16, 16, 8>() &&
              fft_shape_is<4096, 1, 16, 16, 16>(), "FftShape: float32");
static_assert(fft_shape_is<128, 16, 16, 8, 1, double>() && fft_shape_is<256, 8, 16, 16, 1, double>() &&
              fft_shape_is<512, 4, 8, 8, 8, double>() && fft_shape_is<1024, 2, 16, 8, 8, double>() &&
              fft_shape_is<2048, 1, 16, 16, 8, double>(), "FftShape: float64");

// slot of length L in a table whose first length is LMIN (L = LMIN << slot)
constexpr int fft_slot(int64_t L, int LMIN) { return L <= LMIN ? 0 : 1 + fft_slot(L >> 1, LMIN); }

// f(FftLen<LMIN << slot>{}): the run-time slot as a compile-time length, in kernels and launchers alike. The last
// length is the switch's default (a slot is a table index the caller made). A switch, and f by value: a chain of
// comparisons, or f by reference, and the compiler lays the tile kernels out differently from the code that was measured.
template <int V> struct FftLen { static constexpr int value = V; };
template <int LMIN, int LMAX, typename F>
__host__ __device__ __forceinline__ void fft_switch(int slot, F f) {
    static_assert((LMIN << 6) >= LMAX, "fft_switch: seven lengths at most");
    switch (slot) {
        case 0: if constexpr ((LMIN << 0) < LMAX) { f(FftLen<(LMIN << 0)>{}); break; }
        case 1: if constexpr ((LMIN << 1) < LMAX) { f(FftLen<(LMIN << 1)>{}); break; }
        case 2: if constexpr ((LMIN << 2) < LMAX) { f(FftLen<(LMIN << 2)>{}); break; }
        case 3: if constexpr ((LMIN << 3) < LMAX) { f(FftLen<(LMIN << 3)>{}); break; }
        case 4: if constexpr ((LMIN << 4) < LMAX) { f(FftLen<(LMIN << 4)>{}); break; }
        case 5: if constexpr ((LMIN << 5) < LMAX) { f(FftLen<(LMIN << 5)>{}); break; }
        default: f(FftLen<LMAX>{});
    }
}
// host: rc = f(FftLen<L>{}) for a run-time length; one outside the table is an internal error, not another kernel
template <int LMIN, int LMAX, typename F>
int fft_dispatch(int64_t L, F&& f) {
    SSQ_REQUIRE(L >= LMIN && L <= LMAX && !(L & (L - 1)), "no LDS transform of %lld points (%d .. %d)", (long long)L, LMIN, LMAX);
    int rc = 0;
    fft_switch<LMIN, LMAX>(fft_slot(L, LMIN), [&](auto len) { rc = f(len); });
    return rc;
}

// e^{2 pi i q / L}, q < L, appended to `tw` as float pairs: the host form of lds_ifft's twiddle table
inline void fft_twiddles(int L, std::vector<float>& tw) {
    for (int q = 0; q < L; ++q) {
        const double a = 6.283185307179586 * (double)q / (double)L;
        tw.push_back((float)std::cos(a)); tw.push_back((float)std::sin(a));
    }
}

// One L-point inverse FFT per column for G = NT * 16 / L columns, Stockham autosort, LDS [q][g]; radices: FftShape<L>.
// `v` holds the pass-1 inputs on entry (butterfly u = idx / G, column g = idx % G,
// idx = tid + it*NT, input t at q = u + t*L/R1) and the final-pass outputs on exit
// (n_hi = u + t*L/RL with RL the last radix, same idx -> (u, g) mapping).
// EARLY_TW (float32): the twiddles of passes 2 and 3 are requested before the barrier in front of the pass instead of
// after its LDS reads -- the table reads' latency runs under the barrier (block rows 58.9 -> 56.7 us at config 2; no
// change for the intermediates' kernels, which wait on HBM). FRESH: `buf` holds nothing a wavefront may still be
// reading (a kernel's first transform): no barrier before pass 1. TWS: the twiddle table is e^{2 pi i q / (L TWS)} --
// a longer transform's table read at every TWS-th entry (the sub-transforms of block_spectra_multi_kernel). NTH: the
// workgroup's thread count when it is not the geometry's 256 / 128 (16 points per thread all the same; G follows).
template <int L, bool EARLY_TW = false, bool FRESH = false, int TWS = 1, int NTH = 0, typename R>
__device__ __forceinline__ void lds_ifft(cx<R> (&v)[PPT], cx<R>* __restrict__ buf,
                                         const cx<R>* __restrict__ ftw, int tid) {
    constexpr int NT = NTH ? NTH : FftGeom<R>::NT, G = NT * PPT / L;
    constexpr int R1 = FftShape<L, R>::R1, R2 = FftShape<L, R>::R2, R3 = FftShape<L, R>::R3;
    static_assert(L * G == NT * PPT, "L * G must fill the workgroup");
    constexpr bool three = (R3 > 1);
    constexpr bool ETW = EARLY_TW && sizeof(R) == 4;
    if constexpr (!FRESH) __syncthreads();         // LDS free (previous transform's reads done)
    // ---- pass 1 (Ns = 1): inputs already in registers
    {
        constexpr int NB = PPT / R1;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            cx<R> t[R1];
#pragma unroll
            for (int k = 0; k < R1; ++k) t[k] = v[it * R1 + k];
            Dft<R1>::run(t);
            int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < R1; ++k) buf[(u * R1 + k) * G + g] = t[k];
        }
    }
    cx<R> tw2[ETW ? PPT / R2 : 1][ETW ? R2 : 1];
    if constexpr (ETW) {
        constexpr int NB = PPT / R2, Ns = R1, TW = L / (Ns * R2);
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int kk = ((tid + it * NT) / G) % Ns;
#pragma unroll
            for (int k = 1; k < R2; ++k) tw2[it][k] = ftw[kk * k * TW * TWS];
        }
    }
    __syncthreads();
    // ---- pass 2 (Ns = R1)
    {
        constexpr int NB = PPT / R2, Ns = R1, STR = L / R2;
        cx<R> t[NB][R2];
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < R2; ++k) t[it][k] = buf[(u + k * STR) * G + g];
        }
        if (three) __syncthreads();                // in-place: all reads before any write
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            int idx = tid + it * NT, g = idx % G, u = idx / G;
            int kk = u % Ns;
            constexpr int TW = L / (Ns * R2);
#pragma unroll
            for (int k = 1; k < R2; ++k) t[it][k] = cmul_v(t[it][k], ETW ? tw2[ETW ? it : 0][ETW ? k : 0] : ftw[kk * k * TW * TWS]);
            Dft<R2>::run(t[it]);
            if (three) {
                int j0 = (u / Ns) * Ns * R2 + kk;
#pragma unroll
                for (int k = 0; k < R2; ++k) buf[(j0 + k * Ns) * G + g] = t[it][k];
            } else {
#pragma unroll
                for (int k = 0; k < R2; ++k) v[it * R2 + k] = t[it][k];
            }
        }
    }
    if constexpr (three) {
        cx<R> tw3[ETW ? PPT / R3 : 1][ETW ? R3 : 1];
        if constexpr (ETW) {
#pragma unroll
            for (int it = 0; it < PPT / R3; ++it) {
                const int kk = ((tid + it * NT) / G) % (R1 * R2);
#pragma unroll
                for (int k = 1; k < R3; ++k) tw3[it][k] = ftw[kk * k * TWS];
            }
        }
        __syncthreads();
        constexpr int NB = PPT / R3, Ns = R1 * R2, STR = L / R3;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            int idx = tid + it * NT, g = idx % G, u = idx / G;
            cx<R> t[R3];
#pragma unroll
            for (int k = 0; k < R3; ++k) t[k] = buf[(u + k * STR) * G + g];
            int kk = u % Ns;                       // == u (Ns*R3 == L)
#pragma unroll
            for (int k = 1; k < R3; ++k) t[k] = cmul_v(t[k], ETW ? tw3[ETW ? it : 0][ETW ? k : 0] : ftw[kk * k * TWS]);
            Dft<R3>::run(t);
#pragma unroll
            for (int k = 0; k < R3; ++k) v[it * R3 + k] = t[k];
        }
    }
}

// Two transforms of the same shape as a pair (float32; the block rows' Wx and dWx): `lds_ifft<L, true, true>(vw)` and then
// `lds_ifft<L, true>(vd)`, with each pass' twiddles loaded once and its LDS addresses formed once for both planes. Per
// plane the butterflies, their operands and their order are lds_ifft's, so every output bit is. Both planes go through
// the one buffer inside a pass -- write W, barrier, read W, barrier, write D, barrier, read D -- which takes the seven
// barriers the two calls take (three passes; three for two passes), and one plane's butterflies are issued while the
// other plane's points are on their way through the buffer: behind its write and ahead of the barrier that follows.
// As there: the twiddles of passes 2 and 3 are requested ahead of a barrier in front of them. FRESH: `buf` holds nothing
// a wavefront may still be reading on entry; false (the block rows keep their staged band in it): one more barrier, behind
// pass 1's butterflies of W and in front of the pass' first store.
// The buffer is padded: point i sits at i + 2 (i / 32) when a workgroup has G <= 8 columns (`lds_ifft2_points<L>`
// elements instead of 4096). Unpadded, the 16 lanes a `ds_write_b64` serves together write pass 1's outputs R1 G
// points apart (G = 2: 256 B, eight lanes on each bank; G = 4: four) -- more than half of the kernel's LDS cycles went
// to those conflicts; padded, every access of the passes is conflict-free at G <= 4. All strides stay compile-time offsets.
constexpr int lds_ifft2_pad(int L) { return (FftGeom<float>::D / L <= 8) ? 2 : 0; }
template <int L> constexpr int lds_ifft2_points = FftGeom<float>::D + lds_ifft2_pad(L) * (FftGeom<float>::D / 32);
template <int L, bool FRESH = true>
__device__ __forceinline__ void lds_ifft2(cx<float> (&vw)[PPT], cx<float> (&vd)[PPT], cx<float>* __restrict__ buf,
                                          const cx<float>* __restrict__ ftw, int tid) {
    using C = cx<float>;
    constexpr int NT = FftGeom<float>::NT, G = NT * PPT / L;
    constexpr int R1 = FftShape<L>::R1, R2 = FftShape<L>::R2, R3 = FftShape<L>::R3;
    constexpr bool three = (R3 > 1);
    constexpr int NB1 = PPT / R1, NB2 = PPT / R2, STR2 = L / R2;
    // slot of point i, and of a compile-time stride added to it (a multiple of 32 points, or one that stays inside i's 32)
    constexpr int PADE = lds_ifft2_pad(L);
    static_assert(L >= 128 && (R1 * G) % 32 == 0 && 32 % (G < 32 ? G : 32) == 0, "lds_ifft2: strides and the padding");
    auto slot = [](int i) { return i + PADE * (i >> 5); };
#define SSQ_PADDED(o) ((o) + PADE * ((o) >> 5))
    // butterflies of one pass on one plane, in place: radix RR, twiddles tw[it][1 .. RR-1] (none: pass 1)
    auto butterflies = [](auto rr, C (&v)[PPT], auto* tw) {
        constexpr int RR = decltype(rr)::value;
#pragma unroll
        for (int it = 0; it < PPT / RR; ++it) {
            C t[RR];
            t[0] = v[it * RR];
#pragma unroll
            for (int k = 1; k < RR; ++k) {
                if constexpr (std::is_same_v<decltype(tw), std::nullptr_t*>) t[k] = v[it * RR + k];
                else t[k] = cmul_v(v[it * RR + k], tw[it][k]);
            }
            Dft<RR>::run(t);
#pragma unroll
            for (int k = 0; k < RR; ++k) v[it * RR + k] = t[k];
        }
    };
    constexpr std::nullptr_t* none = nullptr;
    int w1[NB1], r2[NB2];                          // first slot a pass-1 butterfly writes, a pass-2 butterfly reads
#pragma unroll
    for (int it = 0; it < NB1; ++it) { const int idx = tid + it * NT; w1[it] = slot((idx / G) * R1 * G + idx % G); }
#pragma unroll
    for (int it = 0; it < NB2; ++it) { const int idx = tid + it * NT; r2[it] = slot(idx); }
    auto put1 = [&](const C (&v)[PPT]) {
#pragma unroll
        for (int it = 0; it < NB1; ++it)
#pragma unroll
            for (int k = 0; k < R1; ++k) buf[w1[it] + SSQ_PADDED(k * G)] = v[it * R1 + k];
    };
    auto get2 = [&](C (&v)[PPT]) {
#pragma unroll
        for (int it = 0; it < NB2; ++it)
#pragma unroll
            for (int k = 0; k < R2; ++k) v[it * R2 + k] = buf[r2[it] + SSQ_PADDED(k * STR2 * G)];
    };
    // ---- pass 1 (Ns = 1) in registers; W out, D's butterflies on the way to the barrier
    butterflies(FftLen<R1>{}, vw, none);
    if constexpr (!FRESH) __syncthreads();         // every wavefront is through with what `buf` held
    put1(vw);
    C tw2[NB2][R2];
#pragma unroll
    for (int it = 0; it < NB2; ++it) {
        const int kk = ((tid + it * NT) / G) % R1;
        constexpr int TW = L / (R1 * R2);
#pragma unroll
        for (int k = 1; k < R2; ++k) tw2[it][k] = ftw[kk * k * TW];
    }
    butterflies(FftLen<R1>{}, vd, none);
    __syncthreads();
    get2(vw);
    __syncthreads();
    put1(vd);
    // ---- pass 2 (Ns = R1): W's butterflies while D goes through the buffer
    butterflies(FftLen<R2>{}, vw, tw2);
    __syncthreads();
    get2(vd);
    if constexpr (!three) {
        butterflies(FftLen<R2>{}, vd, tw2);
    } else {
        constexpr int NB3 = PPT / R3, STR3 = L / R3;
        int w2[NB2], r3[NB3];
#pragma unroll
        for (int it = 0; it < NB2; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
            w2[it] = slot(((u / R1) * R1 * R2 + u % R1) * G + g);
        }
#pragma unroll
        for (int it = 0; it < NB3; ++it) { const int idx = tid + it * NT; r3[it] = slot(idx); }
        auto put2 = [&](const C (&v)[PPT]) {
#pragma unroll
            for (int it = 0; it < NB2; ++it)
#pragma unroll
                for (int k = 0; k < R2; ++k) buf[w2[it] + SSQ_PADDED(k * R1 * G)] = v[it * R2 + k];
        };
        auto get3 = [&](C (&v)[PPT]) {
#pragma unroll
            for (int it = 0; it < NB3; ++it)
#pragma unroll
                for (int k = 0; k < R3; ++k) v[it * R3 + k] = buf[r3[it] + SSQ_PADDED(k * STR3 * G)];
        };
        __syncthreads();                           // in place: every read of D before any write
        put2(vw);
        butterflies(FftLen<R2>{}, vd, tw2);
        C tw3[NB3][R3];
#pragma unroll
        for (int it = 0; it < NB3; ++it) {
            const int kk = ((tid + it * NT) / G) % (R1 * R2);
#pragma unroll
            for (int k = 1; k < R3; ++k) tw3[it][k] = ftw[kk * k];
        }
        __syncthreads();
        get3(vw);
        __syncthreads();
        put2(vd);
        // ---- pass 3 (Ns = R1 R2)
        butterflies(FftLen<R3>{}, vw, tw3);
        __syncthreads();
        get3(vd);
        butterflies(FftLen<R3>{}, vd, tw3);
    }
#undef SSQ_PADDED
}

}  // namespace ssq
