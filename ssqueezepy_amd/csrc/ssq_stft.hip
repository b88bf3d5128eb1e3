// ssq_stft.hip -- STFT / synchrosqueezed-STFT plan (C ABI: ssq_stft_*).
//
// Data flow per signal (reference: ssqueezepy/_stft.py:127-147,166-170,
// _ssq_stft.py:88-122):
//   x (N) --pad_kernel--> xp (N + n_fft - 1)
//   xp --frame_window_kernel--> frames[c][r] = xp[frame c, sample r] * window[r]
//        (and the same with diff_window), frame-major so each transform is contiguous
//   frames --rocFFT R2C, batch = n_hops, output stride n_hops--> Sx[f][c], dSx[f][c]
//        (the strided store writes the (rows, n_hops) layout directly: no transpose)
//   Sx, dSx --accumulate_tile_kernel (STFT form)--> Tx
// float32 with a power-of-two n_fft in [128, 2048] takes the fused kernel instead:
// framing, both windows and both transforms in ONE launch for the whole batch -- the
// two real frames a = frame*window, b = frame*diff_window ride one complex LDS FFT as
// a + ib and are separated by Hermitian symmetry (stft_fused_kernel below).
// The backward pass (ssq_stft_adjoint: gSx, gdSx -> gx) is at the end: stft_adjoint_fused_kernel for the fused plans,
// the composed route of ssq_inverse.hip for the others, one unpadding pass for both.
// Compiled with -ffp-contract=off (see ssq_kernels.hip).
#include "ssq_common.h"
#include "ssq_fft.h"
#include "ssq_ldsfft.h"
#include "ssq_stft.h"
#include <vector>
#include <cmath>
#include <algorithm>
#include <map>
#include <mutex>

namespace ssq {

#include "ssq_point_math.inl"

typedef float ssq_f4 __attribute__((ext_vector_type(4)));
typedef float ssq_f4a4 __attribute__((ext_vector_type(4), aligned(4)));     // 16 bytes at a sample's 4-byte boundary

template <typename T>
__global__ __launch_bounds__(256) void frame_window_kernel(
    const T* __restrict__ xp, const T* __restrict__ window, const T* __restrict__ diff_window,
    T* __restrict__ frames, T* __restrict__ dframes, int64_t n_fft, int64_t n_hops, int64_t hop,
    int64_t s20, int64_t s21, int modulated) {
    const int64_t total = n_fft * n_hops;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = t % n_fft, c = t / n_fft;
        int64_t start = hop * c, s;
        if (!modulated) s = start + r;
        else if (r < s20) s = start + s21 + r;
        else s = start + (r - s20);
        T v = xp[s];
        frames[t] = v * window[r];
        if (dframes) dframes[t] = v * diff_window[r];
    }
}

// ---- fused framing + window + FFT (float32, n_fft = L a power of two) -----------------
// One item = G = 4096/L consecutive frames of one signal. The forward transform is
// taken as conj(IFFT(conj(.))) with the inverse LDS FFT of ssq_ldsfft.h: input
// a - ib, output Z' with FFT(a + ib) = conj(Z'). With A = FFT(a), B = FFT(b) Hermitian,
//   A[f] = (Z[f] + conj(Z[L-f])) / 2,   B[f] = (Z[f] - conj(Z[L-f])) / (2i),  f <= L/2.
// Round 6 (profiles/r6_ab_history.txt "r6w".."r6y"): the Tx planes take the FFT buffer's place (four workgroups per CU);
// the item's samples come through LDS in one coalesced pass; the tables an item needs (window pairs, row frequencies,
// weights) are asked for a phase ahead of their use. Persistent workgroups that fetch the next item's samples while they
// transform the current one were built and measured slower (the loop costs 40 registers: three workgroups per CU).
// What the kernel is NOT bound by, each measured ("r6y8".."r6y11"): a fifth workgroup per CU (the last row of the planes
// kept in registers, LDS exactly 32 KB: no change), its 32-byte output pieces (the same bytes as full lines: -4 %), the
// transform's LDS bank conflicts (padded columns: +2 %). The counters put the vector ALU at ~60 % and the LDS pipe at
// ~58 % busy: what is left is instruction count.

// IADJ (the backward of the fused inverse STFT, ssq_istft_adjoint): the transform is the adjoint of an inverse real
// transform -- every bin leaves with its weight c_k / L (c_k = 1 for DC and Nyquist, 2 elsewhere) and the imaginary
// parts of DC and Nyquist as exact zeros, applied where the bin is stored. `if constexpr`: the other instantiations
// compile to the code they had.
template <int L, bool REASSIGN, bool CST64, bool IADJ = false>
__global__ __launch_bounds__(NT) void stft_fused_kernel(StftFusedArgs A, SsqParams sp) {
    using S = FftShape<L>;
    constexpr int G = S::G, R1 = S::R1, RL = S::RL;
    static_assert(!IADJ || !REASSIGN, "stft_fused_kernel: the inverse's backward stores Sx only");
    // the frames' Tx: a real and an imaginary plane of (L/2 + 1) x G float64 cells. The planes take the FFT buffer's
    // place once its last reader is done (the workgroup's LDS stays at 32 KB + 16 G bytes: four workgroups per CU)
    constexpr int CELLS = REASSIGN ? (L / 2 + 1) * G : 1;
    constexpr int RAW = REASSIGN && 2 * CELLS > D_POINTS ? 2 * CELLS : D_POINTS;
    __shared__ double raw[RAW];
    c32* const buf = reinterpret_cast<c32*>(raw);
    double* const txt = raw;
    float* const sm = reinterpret_cast<float*>(raw);
    static_assert(sizeof(double) * RAW <= 40 * 1024, "stft_fused_kernel: static LDS beyond a quarter of a gfx950 CU's 160 KB");
    constexpr int NI = ((L / 2 + 1) * G + NT - 1) / NT;       // epilogue points per work-item
    using w_t = typename std::conditional<CST64, double, float>::type;
    const int tid = threadIdx.x;
    const bool deriv = A.dSx != nullptr || A.kidx != nullptr || REASSIGN;
    // The item's frames overlap (hop < L): their samples, hop (G - 1) + L of them, come in ONE coalesced pass -- global
    // -> LDS (the FFT buffer, idle until the first pass) -> registers -- instead of 16 four-byte loads per work-item
    // that touch G separate runs each. Frames too far apart for the buffer, and the padded-copy route, read global
    // memory directly as before.
    const int span = A.hop * (G - 1) + L;
    const bool staged = A.x != nullptr && span <= 2 * D_POINTS;
    // modulated: the frame is rotated by n_fft / 2 (utils/stft_utils.py:76-82) -- L is even: an XOR
    const int rot = A.modulated ? L / 2 : 0;
    // the items (signal, group of G frames), frames fastest. Workgroups are dealt to the 8 XCDs round-robin: each XCD
    // takes one contiguous range of items, so that the G*8-byte pieces of an output line meet in one L2 before they leave
    const int ng = (int)((A.n_hops + G - 1) / G);
    const int64_t total = (int64_t)ng * A.batch;
    int64_t item = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (A.xcd) {
        const int64_t nwg = (int64_t)gridDim.x * gridDim.y, per = nwg >> 3;       // (the launch pads nwg to a multiple of 8)
        item = (item & 7) * per + (item >> 3);
    }
    if (item >= total) return;
    {
        const int b = (int)(item / ng), c0 = (int)(item % ng) * G;
        const int t0 = A.hop * c0 - A.n1;                      // the first sample's index in the signal
        // (frames inside the signal read it directly -- all but the items at its two ends, padded on the fly)
        const bool inside = A.x != nullptr && t0 >= 0 && t0 + span - 1 < A.n;
        c32 z[PPT];
        if (staged) {
            // (the window pairs are asked for before the samples: their latency passes behind the staging barrier --
            // phase stamps, "r6x": reading them after it was a quarter of a workgroup's life)
            constexpr int NB = PPT / R1, STR = L / R1;
            float2 wv[PPT];
#pragma unroll
            for (int it = 0; it < NB; ++it) {
#pragma unroll
                for (int k = 0; k < R1; ++k) {
                    const int r = (tid + it * NT) / G + k * STR;
                    if (deriv && A.wd) wv[it * R1 + k] = A.wd[r];
                    else wv[it * R1 + k] = make_float2(A.window[r], 0.f);
                }
            }
            const float* xb = A.x + (int64_t)b * A.n;
            if (inside) {
                for (int i = tid * 4; i < span; i += NT * 4) {
                    if (i + 4 <= span) *reinterpret_cast<ssq_f4*>(sm + i) = *reinterpret_cast<const ssq_f4a4*>(xb + t0 + i);
                    else for (int q = i; q < span; ++q) sm[q] = xb[t0 + q];
                }
            } else {
                for (int i = tid; i < span; i += NT) {
                    const int src = stft_pad_source(t0 + i, A.n, A.padtype);
                    sm[i] = src < 0 ? 0.f : xb[src];
                }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NB; ++it) {
                const int idx = tid + it * NT, g = idx % G, u = idx / G;
                const bool live = c0 + g < A.n_hops;
                const float* fr = sm + A.hop * g;
#pragma unroll
                for (int k = 0; k < R1; ++k) {
                    const int r = u + k * STR;                // sample of the frame
                    const float v = live ? fr[r ^ rot] : 0.f;
                    z[it * R1 + k] = {v * wv[it * R1 + k].x, -(v * wv[it * R1 + k].y)};
                }
            }
            __syncthreads();                                   // the samples are in registers: the buffer is the FFT's
        } else {
            const float* xp = A.xp + (int64_t)b * A.padlen;
            const float* xs = A.x + (int64_t)b * A.n - A.n1;
            constexpr int NB = PPT / R1, STR = L / R1;
#pragma unroll
            for (int it = 0; it < NB; ++it) {
                const int idx = tid + it * NT, g = idx % G, u = idx / G;
                const int c = c0 + g;
#pragma unroll
                for (int k = 0; k < R1; ++k) {
                    const int r = u + k * STR;                // sample of the frame
                    const int s = r ^ rot;
                    float a = 0.f, bb = 0.f;
                    if (c < A.n_hops) {
                        float v;
                        if (inside) v = xs[A.hop * c + s];     // (item-uniform: every sample of its frames exists)
                        else if (A.x) {                        // the signal's ends: padded on the fly
                            const int src = stft_pad_source(A.hop * c + s - A.n1, A.n, A.padtype);
                            v = src < 0 ? 0.f : A.x[(int64_t)b * A.n + src];
                        } else v = xp[(int64_t)A.hop * c + s];
                        a = v * A.window[r];
                        if (deriv) bb = v * A.diff_window[r];
                    }
                    z[it * R1 + k] = {a, -bb};
                }
            }
        }
        // the rows' frequencies of the epilogue's points (and the weight of the reference's linear grid -- a weight
        // vector is read where it is used) are asked for here, a transform ahead of their use
        float sf[REASSIGN ? NI : 1]; w_t cw0 = 0;
        if constexpr (REASSIGN) {
#pragma unroll
            for (int it = 0; it < NI; ++it) sf[it] = A.Sfs[min((tid + it * NT) / G, L / 2)];
            cw0 = ((const w_t*)A.cst)[0];
        }
        // (FRESH: a barrier has just passed; the twiddles asked for ahead of each pass' barrier measured no gain here)
        lds_ifft<L, false, true>(z, buf, A.ftw, tid);
        __syncthreads();                              // last pass' LDS reads are done
        {
            constexpr int NB = PPT / RL, STR = L / RL;
#pragma unroll
            for (int it = 0; it < NB; ++it) {
                const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
                for (int k = 0; k < RL; ++k) buf[(u + k * STR) * G + g] = z[it * RL + k];
            }
        }
        __syncthreads();
        const int64_t base = (int64_t)b * A.rows * A.n_hops;
        if constexpr (!REASSIGN) {
            for (int i = tid; i < (L / 2 + 1) * G; i += NT) {
                const int f = i / G, g = i % G, c = c0 + g;
                if (c >= A.n_hops) continue;
                const c32 P = buf[f * G + g], Q = buf[((L - f) & (L - 1)) * G + g];
                const int64_t q = base + (int64_t)f * A.n_hops + c;
                float sr = 0.5f * (P.x + Q.x), si = 0.5f * (Q.y - P.y);
                if constexpr (IADJ) {
                    const bool edge = f == 0 || f == L / 2;
                    const float c = edge ? 1.f / L : 2.f / L;
                    sr = sr * c; si = edge ? 0.f : si * c;
                }
                A.Sx[q] = make_float2(sr, si);
                if (!deriv) continue;
                const float dr = -0.5f * (P.y + Q.y), di = 0.5f * (Q.x - P.x);
                if (A.dSx) A.dSx[q] = make_float2(dr, di);
                if (A.kidx) {   // the fused kernels' rule (algos.py:956-984): |Sx| > gamma, then the bin
                    const int64_t omax = A.rows - 1;
                    unsigned short kk = 0xFFFFu;
                    if (mag_gt(sr, si, A.gamma)) {
                        const int64_t kb = bin_of_point(dr, di, sr, si, true, A.Sfs[f], sp, omax);
                        kk = (unsigned short)(sp.flipud ? omax - kb : kb);
                    }
                    A.kidx[q] = kk;
                }
            }
        } else {
            // every point of the item's frames leaves the FFT buffer for registers (its Sx on the way to HBM, its bin
            // beside it) before the buffer becomes the Tx planes. No early-outs: a point outside the frames, or below
            // gamma, carries the bin 0xFFFF
            float vr[NI], vi[NI]; unsigned kq[NI];
            const int omax = (int)A.rows - 1;
#pragma unroll
            for (int it = 0; it < NI; ++it) {
                const int i = tid + it * NT, f = min(i / G, L / 2), g = i % G, c = c0 + g;
                const bool valid = i < (L / 2 + 1) * G && c < A.n_hops;
                const c32 P = buf[f * G + g], Q = buf[((L - f) & (L - 1)) * G + g];
                const float sr = 0.5f * (P.x + Q.x), si = 0.5f * (Q.y - P.y);
                const float dr = -0.5f * (P.y + Q.y), di = 0.5f * (Q.x - P.x);
                if (valid) {
                    A.Sx[base + (int64_t)f * A.n_hops + c] = make_float2(sr, si);
                    if (A.dSx) A.dSx[base + (int64_t)f * A.n_hops + c] = make_float2(dr, di);
                }
                // the fused kernels' rule (algos.py:956-984): |Sx| > gamma, then the bin
                const bool on = valid && mag_gt(sr, si, A.gamma);
                const int kb = bin_of_point_stft(dr, di, sr, si, sf[it], sp, omax, on);
                kq[it] = on ? (unsigned)(sp.flipud ? omax - kb : kb) : 0xFFFFu;
                vr[it] = sr; vi[it] = si;
                if (it % 3 == 2) SSQ_SCHED_FENCE();            // (three points' LDS reads in flight, not all nine)
            }
            __syncthreads();                              // the buffer's last read
            for (int i = tid; i < 2 * CELLS; i += NT) txt[i] = 0.0;
            __syncthreads();
#pragma unroll
            for (int it = 0; it < NI; ++it) {
                if (kq[it] == 0xFFFFu) continue;
                const int g = (tid + it * NT) % G;
                // the term in the CPU path's arithmetic (float32 product; float64 with a float64 weight vector), the
                // sum in float64
                const w_t cw = A.cst_uniform ? cw0 : ((const w_t*)A.cst)[min((tid + it * NT) / G, L / 2)];
                const double tr = (double)((w_t)vr[it] * cw), ti = (double)((w_t)vi[it] * cw);
                const unsigned off = (kq[it] * G + (unsigned)g) * 8u;
                SSQ_LDS_ADD_F64(txt, off, tr);
                SSQ_LDS_ADD_F64(txt, off + (unsigned)CELLS * 8u, ti);
            }
            __syncthreads();
            for (int i = tid; i < (L / 2 + 1) * G; i += NT) {
                const int f = i / G, g = i % G, c = c0 + g;
                if (c >= A.n_hops) continue;
                A.Tx[base + (int64_t)f * A.n_hops + c] = make_float2((float)txt[i], (float)txt[CELLS + i]);
            }
        }
    }
}

// one workgroup per item; the grid is two-dimensional only to hold more than 2^31 - 1 of them
template <int L, bool IADJ = false>
static int launch_stft_fused(const StftFusedArgs& A, const SsqParams& sp, int64_t batch, hipStream_t stream) {
    constexpr int G = FftShape<L>::G;
    SSQ_REQUIRE(!A.Tx || A.rows == L / 2 + 1, "fused reassignment: %lld rows, transform of %d", (long long)A.rows, L);
    StftFusedArgs B = A;
    B.batch = (int)batch;
    int64_t total = (int64_t)((A.n_hops + G - 1) / G) * batch;
    B.xcd = total >= 64;
    if (B.xcd) total = (total + 7) & ~(int64_t)7;
    // (grid.x a multiple of 8 when the items are remapped, so that the product is one too)
    const int64_t gx = std::min<int64_t>(total, (int64_t)1 << 20), gy = (total + gx - 1) / gx;
    SSQ_REQUIRE(gy <= 65535, "stft_fused_kernel: %lld items", (long long)total);
    dim3 grid((unsigned)gx, (unsigned)gy);
    if constexpr (IADJ)
        hipLaunchKernelGGL((stft_fused_kernel<L, false, false, true>), grid, dim3(NT), 0, stream, B, sp);
    else if (!A.Tx)
        hipLaunchKernelGGL((stft_fused_kernel<L, false, false>), grid, dim3(NT), 0, stream, B, sp);
    else if (sp.cst_f64)
        hipLaunchKernelGGL((stft_fused_kernel<L, true, true>), grid, dim3(NT), 0, stream, B, sp);
    else
        hipLaunchKernelGGL((stft_fused_kernel<L, true, false>), grid, dim3(NT), 0, stream, B, sp);
    SSQ_LAUNCH_CHECK();
    return 0;
}


// ---- fused adjoint of the STFT (float32, n_fft = L a power of two): gSx, gdSx -> overlap-added frames ------
// One item = `nf` consecutive frames of one signal. Their overlap-added, windowed inverse transforms -- a strip of
// (nf - 1) hop + L padded samples -- are summed in LDS and leave the workgroup once; no frame is ever in HBM, no frame
// is computed twice, and no sum depends on the order workgroups or wavefronts run in (each strip sample belongs to
// one work-item, which adds its frames in ascending order). The strips of neighbouring items overlap by L - hop
// samples: stft_adjoint_unpad_kernel adds them, items ascending, while it folds the padding back onto the signal.
// The real-output transforms ride the complex LDS inverse two at a time, as the forward's two windows do: with A, B
// the Hermitian completions of two half-spectra (interior bins halved, the imaginary parts of DC and Nyquist dropped:
// they do not reach a real output), ifft(A + iB) = a + ib. The pair is (gSx, gdSx) of one frame when both gradients
// are there (G frames a pass), frames j and j + G of the one that is otherwise (2 G frames a pass).
constexpr int ADJ_SPAN = 5120;                       // strip samples: 20 KB beside the transform's 32.5 KB (the LDS would hold three
                                                     // workgroups per CU; from n_fft = 512 on the 186 .. 241 registers allow two)
constexpr int ADJ_RAW = 2 * D_POINTS + 128;          // floats: the FFT buffer, then 2 G windowed frames of pitch L + 64 / G

struct StftAdjArgs {
    const float2* gA; const float2* gB;              // (batch, rows, n_hops); gB null: gA's frames pair up
    const float* winA; const float* winB;            // the windows that go with gA, gB
    const c32* ftw; float* ws;                       // ws (batch, n_items, span)
    int64_t n_hops, rows, n_items;
    int hop, modulated, nf, span, batch;
};

// INV: the same kernel as the fused inverse STFT (ssq_istft_batch). What differs is the weights of an inverse real
// transform -- every bin whole and 1 / L (exact: L is a power of two) where the adjoint halves the interior bins --,
// the window (gA = Sx, winA = window^a in the transform's order, gB null) and the pass that finishes the strips
// (istft_finish_kernel: the window norm and the trim instead of the padding's transpose).
template <int L, bool INV>
__global__ __launch_bounds__(NT) void stft_adjoint_fused_kernel(StftAdjArgs A) {
    using S = FftShape<L>;
    constexpr int G = S::G, R1 = S::R1, RL = S::RL;
    __shared__ float raw[ADJ_RAW];
    __shared__ float strip[ADJ_SPAN];
    constexpr int PITCH = L + 64 / G;                // (the G columns of a butterfly's output land in G different banks)
    static_assert(2 * G * PITCH <= ADJ_RAW, "stft_adjoint_fused_kernel: the windowed frames outgrow the FFT buffer");
    static_assert(sizeof(float) * (ADJ_RAW + ADJ_SPAN) <= 53 * 1024, "stft_adjoint_fused_kernel: static LDS beyond a third of a CU's 160 KB");
    c32* const buf = reinterpret_cast<c32*>(raw);
    const int tid = threadIdx.x;
    const int64_t item = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (item >= A.n_items * A.batch) return;
    const int b = (int)(item / A.n_items), it0 = (int)(item % A.n_items);
    const int64_t c_first = (int64_t)it0 * A.nf;
    const int nfv = A.n_hops - c_first < A.nf ? (int)(A.n_hops - c_first) : A.nf;          // the item's frames
    const bool both = A.gB != nullptr;
    const int FP = both ? G : 2 * G;                                       // frames per pass
    const float2* const gB = both ? A.gB : A.gA;
    const int rot = A.modulated ? L / 2 : 0;
    const int64_t base = (int64_t)b * A.rows * A.n_hops + c_first;
    const int span = (nfv - 1) * A.hop + L;                                // <= A.span <= ADJ_SPAN
    for (int p = tid; p < span; p += NT) strip[p] = 0.f;                  // (strip[p] is work-item p % NT's alone)
    for (int j0 = 0; j0 < nfv; j0 += FP) {
        const int fpv = min(FP, nfv - j0);
        c32 z[PPT];
        {
            constexpr int NB = PPT / R1, STR = L / R1;
#pragma unroll
            for (int it = 0; it < NB; ++it) {
                const int idx = tid + it * NT, g = idx % G, u = idx / G;
                const int jA = j0 + g, jB = both ? jA : jA + G;
#pragma unroll
                for (int k = 0; k < R1; ++k) {
                    const int q = u + k * STR, f = q <= L / 2 ? q : L - q;
                    const bool edge = f == 0 || f == L / 2;
                    const int64_t row = base + (int64_t)f * A.n_hops;
                    float2 a = make_float2(0.f, 0.f), d = make_float2(0.f, 0.f);
                    if (jA < nfv) a = A.gA[row + jA];
                    if (jB < nfv) d = gB[row + jB];
                    constexpr float WI = INV ? 1.f / L : 0.5f, WE = INV ? 1.f / L : 1.f;      // interior, edge bins
                    const float s = edge ? WE : WI, si = edge ? 0.f : (q > L / 2 ? -WI : WI);
                    const float ar = a.x * s, ai = a.y * si, br = d.x * s, bi = d.y * si;
                    z[it * R1 + k] = {ar - bi, ai + br};
                }
            }
        }
        lds_ifft<L>(z, buf, A.ftw, tid);     // (its first barrier: the last pass' frames are read)
        __syncthreads();                                                   // the transform's LDS reads are done
        {
            constexpr int NB = PPT / RL, STR = L / RL;
#pragma unroll
            for (int it = 0; it < NB; ++it) {
                const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
                for (int k = 0; k < RL; ++k) {
                    const int n = u + k * STR;
                    const c32 v = z[it * RL + k];
                    if (both) raw[g * PITCH + n] = v.x * A.winA[n] + v.y * A.winB[n];
                    else {
                        raw[g * PITCH + n] = v.x * A.winA[n];
                        raw[(G + g) * PITCH + n] = v.y * A.winA[n];
                    }
                }
            }
        }
        __syncthreads();
        // the pass' frames j0 .. j0 + fpv - 1 into the strip: sample p takes frame j's sample p - j hop
        const int p_lo = j0 * A.hop, p_hi = (j0 + fpv - 1) * A.hop + L;
        for (int p = p_lo + ((tid - p_lo) & (NT - 1)); p < p_hi; p += NT) {
            const int j_hi = min(j0 + fpv - 1, p / A.hop);
            const int j_lo = max(j0, p < L ? 0 : (p - L) / A.hop + 1);
            float acc = strip[p];
            for (int j = j_lo; j <= j_hi; ++j) acc = acc + raw[(j - j0) * PITCH + ((p - j * A.hop) ^ rot)];
            strip[p] = acc;
        }
    }
    float* const o = A.ws + ((int64_t)b * A.n_items + it0) * A.span;
    for (int p = tid; p < span; p += NT) o[p] = strip[p];
}

// gx[j] = the sum of the overlap-added samples whose source under the padding rule is j: `off`, `idx` list those
// padded positions per signal sample, ascending. A position is summed over the strips that hold it -- item i holds the
// positions [i step, i step + span) -- items ascending; positions from `pmax` on lie behind the last frame.
template <typename T>
__global__ __launch_bounds__(256) void stft_adjoint_unpad_kernel(
    const T* __restrict__ ws, T* __restrict__ gx, const int32_t* __restrict__ off, const int32_t* __restrict__ idx,
    int64_t n, int64_t n_items, int64_t step, int64_t span, int64_t pmax) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const T* w = ws + (int64_t)blockIdx.y * n_items * span;
    T acc = T(0);
    for (int32_t e = off[j]; e < off[j + 1]; ++e) {
        const int64_t p = idx[e];
        if (p >= pmax) continue;
        const int64_t i_hi = p / step < n_items - 1 ? p / step : n_items - 1, i_lo = p < span ? 0 : (p - span) / step + 1;
        for (int64_t i = i_lo; i <= i_hi; ++i) acc = acc + w[i * span + (p - i * step)];
    }
    gx[(int64_t)blockIdx.y * n + j] = acc;
}

// x[b][s] = the overlap-added sample p = s + half (the trim), summed over the strips that hold it, items ascending, and
// divided by the window norm wn[s] where that is above `tiny` (the reference's window_norm, in double as istft_ola_kernel)
__global__ __launch_bounds__(256) void istft_finish_kernel(const float* __restrict__ ws, const double* __restrict__ wn,
                                                           float* __restrict__ x, int64_t N, int64_t half,
                                                           int64_t n_items, int64_t step, int64_t span, int64_t pmax,
                                                           float tiny) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    const float* w = ws + (int64_t)blockIdx.y * n_items * span;
    const int64_t p = s + half;
    float acc = 0.f;
    if (p < pmax) {
        const int64_t i_hi = p / step < n_items - 1 ? p / step : n_items - 1, i_lo = p < span ? 0 : (p - span) / step + 1;
        for (int64_t i = i_lo; i <= i_hi; ++i) acc = acc + w[i * span + (p - i * step)];
    }
    const double d = wn[s];
    if (d > (double)tiny) acc = (float)((double)acc / d);
    x[(int64_t)blockIdx.y * N + s] = acc;
}

template <int L, bool INV = false>
static int launch_stft_adjoint_fused(const StftAdjArgs& A, hipStream_t stream) {
    const int64_t total = A.n_items * A.batch;
    const int64_t gx = std::min<int64_t>(total, (int64_t)1 << 20), gy = (total + gx - 1) / gx;
    SSQ_REQUIRE(gy <= 65535, "stft_adjoint_fused_kernel: %lld items", (long long)total);
    hipLaunchKernelGGL((stft_adjoint_fused_kernel<L, INV>), dim3((unsigned)gx, (unsigned)gy), dim3(NT), 0,
                       stream, A);
    SSQ_LAUNCH_CHECK();
    return 0;
}

}  // namespace ssq

using namespace ssq;

struct ssq_stft_plan {
    ssq_stft_desc d;
    int64_t padlen = 0, n1 = 0, n2 = 0, rows = 0, n_hops = 0;
    int rsize() const { return d.dtype == SSQ_F32 ? 4 : 8; }
    DeviceArena mem;                              // every device pointer below but the weight versions
    void* window = nullptr; void* diff_window = nullptr;
    void* xp = nullptr; void* frames = nullptr; void* dframes = nullptr; void* dSx_ws = nullptr;
    FftPlan fft;                                  // R2C, transposed output: transform c writes bin f at Sx[f * n_hops + c]
    bool fused = false; void* ftw = nullptr;      // fused float32 path (power-of-two n_fft)
    void* wd = nullptr;                           // ... its (window, diff_window) pairs, one 8-byte load per sample
    // fused float32 path for the other sizes (prime factors <= 31): mixed-radix LDS transform
    bool generic_fused = false; int gen_radix[GEN_MAX_PASSES] = {0}; int gen_npass = 0, gen_G = 0;
    unsigned short* kidx = nullptr;               // bin map of the fused ssq_stft form
    bool have_ssq = false; SsqParams sp{}; void* cst = nullptr; void* Sfs = nullptr;   // current entries of
    WeightVersions weights, freqs;                                                      // these
    PlanOrder order;
    bool executed = false;
    int32_t* adj_off = nullptr; int32_t* adj_idx = nullptr;   // the adjoint's inverse pad map (built at its first call)
};

extern "C" {

int ssq_stft_plan_create(ssq_stft_plan** out, const ssq_stft_desc* desc) {
    SSQ_REQUIRE(out && desc, "ssq_stft_plan_create: null pointer");
    const ssq_stft_desc& d = *desc;
    SSQ_REQUIRE(d.dtype == SSQ_F32 || d.dtype == SSQ_F64, "bad dtype %d", d.dtype);
    SSQ_REQUIRE(d.n >= 1 && d.n_fft >= 1 && d.hop_len >= 1, "bad sizes n=%lld n_fft=%lld hop=%lld",
                (long long)d.n, (long long)d.n_fft, (long long)d.hop_len);
    SSQ_REQUIRE(d.window, "window must not be null");
    SSQ_REQUIRE(d.padtype >= SSQ_PAD_ZERO && d.padtype <= SSQ_PAD_WRAP, "bad padtype %d", d.padtype);
    PlanGuard<ssq_stft_plan> pl(new ssq_stft_plan(), ssq_stft_plan_destroy);
    pl->d = d;
    if (pl->d.max_batch < 1) pl->d.max_batch = 1;
    // padsignal(x, padlength = N + n_fft - 1): even total -> split evenly, odd -> left
    // gets the extra sample (utils/common.py:116-124)
    pl->padlen = d.n + d.n_fft - 1;
    int64_t tot = pl->padlen - d.n;
    pl->n2 = tot / 2;
    pl->n1 = (tot % 2 == 0) ? pl->n2 : pl->n2 + 1;
    pl->rows = d.n_fft / 2 + 1;
    pl->n_hops = (pl->padlen - d.n_fft) / d.hop_len + 1;
    const int rs = pl->rsize();
    DeviceArena& mem = pl->mem;
    int rc;
    if ((rc = mem.upload(&pl->window, d.window, (size_t)d.n_fft * rs))) return rc;
    if (d.diff_window && (rc = mem.upload(&pl->diff_window, d.diff_window, (size_t)d.n_fft * rs))) return rc;
    if ((rc = mem.alloc(&pl->xp, (size_t)pl->d.max_batch * pl->padlen * rs))) return rc;
    const bool own = d.dtype == SSQ_F32 && !getenv("SSQ_DEBUG_STFT_GENERIC");
    const bool pow2 = (d.n_fft & (d.n_fft - 1)) == 0;
    pl->fused = own && pow2 && d.n_fft >= 128 && d.n_fft <= 2048;
    pl->generic_fused = own && !pl->fused && stft_generic_plan(d.n_fft, pl->gen_radix, &pl->gen_npass, &pl->gen_G);
    if (pl->fused || pl->generic_fused) {
        std::vector<float> tw;
        fft_twiddles((int)d.n_fft, tw);
        if ((rc = mem.upload(&pl->ftw, tw.data(), tw.size() * 4))) return rc;
    }
    if (pl->fused && d.diff_window) {
        std::vector<float> wd((size_t)2 * d.n_fft);
        for (int64_t q = 0; q < d.n_fft; ++q) {
            wd[2 * q] = ((const float*)d.window)[q]; wd[2 * q + 1] = ((const float*)d.diff_window)[q];
        }
        if ((rc = mem.upload(&pl->wd, wd.data(), wd.size() * 4))) return rc;
    }
    // The framing workspace (two n_fft x n_hops arrays) and the rocFFT plan belong to the unfused route only: a fused
    // plan does without them (at the reference's hop-1 benchmark shape they would be 2 x 383 MB). The derivative's
    // workspace (dSx not returned, and no bin map in its place) is allocated at the first execute that needs it.
    if (!pl->fused && !pl->generic_fused) {
        const size_t fb = (size_t)d.n_fft * pl->n_hops * rs;
        if ((rc = mem.alloc(&pl->frames, fb))) return rc;
        if ((rc = mem.alloc(&pl->dframes, fb))) return rc;
        rc = pl->fft.create(0, d.dtype, (size_t)d.n_fft, (size_t)pl->n_hops, 1.0, (size_t)d.n_fft, 1, (size_t)pl->n_hops);
        if (rc) return rc;
    }
    pl->d.window = nullptr; pl->d.diff_window = nullptr;
    *out = pl.release();
    return 0;
}

void ssq_stft_plan_destroy(ssq_stft_plan* pl) {
    if (!pl) return;
    pl->fft.destroy();
    pl->weights.destroy(); pl->freqs.destroy(); pl->order.destroy();
    pl->mem.release();
    delete pl;
}

int ssq_stft_plan_set_ssq(ssq_stft_plan* pl, const void* Sfs, int grid, const double* params,
                          const void* cst, int cst_f64, int flipud, double gamma) {
    SSQ_REQUIRE(pl && Sfs && params && cst, "ssq_stft_plan_set_ssq: null pointer");
    SSQ_REQUIRE(grid >= SSQ_GRID_LOG && grid <= SSQ_GRID_LIN, "unknown grid kind %d", grid);
    std::lock_guard<std::mutex> lock(pl->order.mu);
    float cst0;                                            // (the STFT kernels read the weights' table)
    int rc = set_ssq_params(pl->sp, pl->weights, &pl->cst, &cst0, pl->d.dtype, pl->rows, grid, params, cst, cst_f64, flipud,
                            gamma);
    if (rc) return rc;
    rc = pl->freqs.upload(&pl->Sfs, Sfs, (size_t)pl->rows * pl->rsize());
    if (rc) return rc;
    pl->have_ssq = true;
    return 0;
}

const char* ssq_stft_plan_algo(const ssq_stft_plan* pl) {
    return !pl ? "" : pl->fused ? "fused" : pl->generic_fused ? "fused-mixed-radix" : "rocfft";
}

int ssq_stft_generic_shape(int64_t n_fft, int* radix, int* npass, int* G) {
    int r[GEN_MAX_PASSES] = {0}, np = 0, g = 0;
    for (int p = 0; radix && p < GEN_MAX_PASSES; ++p) radix[p] = 0;
    if (npass) *npass = 0;
    if (G) *G = 0;
    const bool pow2 = (n_fft & (n_fft - 1)) == 0;
    if ((pow2 && n_fft >= 128 && n_fft <= 2048) || !stft_generic_plan(n_fft, r, &np, &g)) return 0;
    for (int p = 0; radix && p < np; ++p) radix[p] = r[p];
    if (npass) *npass = np;
    if (G) *G = g;
    return 1;
}

int ssq_stft_plan_shape(const ssq_stft_plan* pl, int64_t* rows, int64_t* n_hops) {
    SSQ_REQUIRE(pl, "ssq_stft_plan_shape: null plan");
    if (rows) *rows = pl->rows;
    if (n_hops) *n_hops = pl->n_hops;
    return 0;
}

}  // extern "C"

template <typename T>
static int stft_execute_t(ssq_stft_plan* pl, const void* x, int64_t batch, void* Sx, void* dSx,
                          void* Tx, void* w, hipStream_t stream) {
    const ssq_stft_desc& d = pl->d;
    const int64_t rows = pl->rows, n_hops = pl->n_hops, n_fft = d.n_fft;
    const bool deriv = dSx || Tx || w;
    SSQ_REQUIRE(!deriv || pl->diff_window, "derivative outputs need a diff_window");
    // (the power-of-two fused kernel pads on the fly; the other routes read a padded copy)
    const bool pad_in_kernel = sizeof(T) == 4 && pl->fused && d.n + pl->n1 + pl->n2 < ((int64_t)1 << 30);
    int rc = 0;
    if (!pad_in_kernel) rc = ssq_pad_signal(d.dtype, x, pl->xp, batch, d.n, pl->n1, pl->n2, d.padtype, stream);
    if (rc) return rc;
    const int64_t s20 = (n_fft + 1) / 2, s21 = (n_fft % 2 == 1) ? s20 - 1 : s20;
    T* dS = (T*)dSx;
    // fused ssq_stft form: Tx wanted, neither dSx nor w -> the kernel emits 2-byte bins
    // instead of the 8-byte derivative (the reassignment then reads 10 instead of 16 B/pt)
    // ... and, unless the ordered sums are asked for (SSQ_TILE_ORDER=ordered), sums Tx itself
    bool use_kidx = false, fused_tx = false;
    if constexpr (sizeof(T) == 4) {
        if ((pl->fused || pl->generic_fused) && Tx && !w && !dSx && rows < 65535) {
            use_kidx = true;
            // (round 6, the Tx planes in the FFT buffer's place, four workgroups per CU: config 3 at 512 signals 1.87 ms
            // against 2.19 with the separate pass, 64 signals 0.26 against 0.31, hop 1 0.83 against 1.02 -- profiles/
            // r6_ab_history.txt "r6w"; the separate pass stays for the ordered sums; SSQ_DEBUG_STFT_FUSED_TX=0/1 forces)
            const char* fe = getenv("SSQ_DEBUG_STFT_FUSED_TX");        // (read at every call, like SSQ_TILE_ORDER: tests switch it)
            const int force = (fe && *fe) ? atoi(fe) : -1;
            fused_tx = !reassign_ordered() && rows == n_fft / 2 + 1 && force != 0;
            if (!fused_tx && !pl->kidx && (rc = pl->mem.alloc(&pl->kidx, (size_t)pl->d.max_batch * rows * n_hops * 2)))
                return rc;
        }
    }
    // the derivative is needed (phase transform / bins) but not returned: its workspace exists from the first such call
    if (deriv && !dSx && !use_kidx) {
        if (!pl->dSx_ws && (rc = pl->mem.alloc(&pl->dSx_ws, (size_t)pl->d.max_batch * rows * n_hops * sizeof(T) * 2)))
            return rc;
        dS = (T*)pl->dSx_ws;
    }
    if constexpr (sizeof(T) == 4) {
        if (pl->fused || pl->generic_fused) {
            StftFusedArgs A;
            A.xp = (const float*)pl->xp; A.window = (const float*)pl->window;
            A.diff_window = (const float*)pl->diff_window;
            A.Sx = (float2*)Sx; A.dSx = (deriv && !use_kidx) ? (float2*)dS : nullptr;
            A.kidx = (use_kidx && !fused_tx) ? pl->kidx : nullptr; A.Sfs = (const float*)pl->Sfs; A.gamma = pl->sp.gamma;
            A.Tx = fused_tx ? (float2*)Tx : nullptr; A.cst = pl->cst; A.cst_uniform = pl->sp.cst_uniform;
            A.padlen = pl->padlen; A.n_hops = n_hops; A.rows = rows;
            A.hop = (int)d.hop_len; A.s20 = (int)s20; A.s21 = (int)s21; A.modulated = d.modulated;
            A.n = (int)d.n; A.n1 = (int)pl->n1; A.padtype = d.padtype;
            if (pl->fused) {                              // (its launch sets xcd and batch)
                A.ftw = (const c32*)pl->ftw; A.x = pad_in_kernel ? (const float*)x : nullptr; A.wd = (const float2*)pl->wd;
                rc = fft_dispatch<128, 2048>(n_fft, [&](auto len) { return launch_stft_fused<decltype(len)::value>(A, pl->sp, batch, stream); });
            } else {                                      // (the twiddles are an argument of its own)
                A.ftw = nullptr; A.x = nullptr; A.wd = nullptr; A.xcd = 0; A.batch = (int)batch;
                rc = launch_stft_generic(A, pl->sp, (const c32*)pl->ftw, (int)n_fft, pl->gen_radix, pl->gen_npass, pl->gen_G,
                                         batch, stream);
            }
            if (rc) return rc;
        }
    }
    if (!pl->fused && !pl->generic_fused) {               // rocFFT route: frames, then one transform per plane and signal
        for (int64_t b = 0; b < batch; ++b) {
            const T* xp = (const T*)pl->xp + (size_t)b * pl->padlen;
            int64_t total = n_fft * n_hops;
            unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
            hipLaunchKernelGGL((frame_window_kernel<T>), dim3(g), dim3(256), 0, stream, xp,
                               (const T*)pl->window, (const T*)pl->diff_window, (T*)pl->frames,
                               deriv ? (T*)pl->dframes : (T*)nullptr, n_fft, n_hops, d.hop_len, s20, s21,
                               d.modulated);
            SSQ_LAUNCH_CHECK();
            T* Sx_b = (T*)Sx + (size_t)b * rows * n_hops * 2;
            rc = pl->fft.execute(pl->frames, Sx_b, stream);
            if (rc) return rc;
            if (deriv) {
                rc = pl->fft.execute(pl->dframes, dS + (size_t)b * rows * n_hops * 2, stream);
                if (rc) return rc;
            }
        }
    }
    if (w) {
        rc = ssq_phase_stft(d.dtype, Sx, dS, pl->Sfs, w, batch, rows, n_hops, pl->sp.gamma, stream);
        if (rc) return rc;
    }
    if (Tx && !fused_tx) {
        if (w)
            rc = launch_accumulate(d.dtype, BIN_FROM_W, Sx, w, nullptr, Tx, pl->cst, pl->sp, batch,
                                   rows, n_hops, nullptr, stream);
        else if (use_kidx)
            rc = launch_accumulate(d.dtype, BIN_FROM_KIDX, Sx, pl->kidx, nullptr, Tx, pl->cst, pl->sp, batch,
                                   rows, n_hops, nullptr, stream);
        else
            rc = launch_accumulate(d.dtype, BIN_FROM_DWX, Sx, dS, pl->Sfs, Tx, pl->cst, pl->sp, batch,
                                   rows, n_hops, nullptr, stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int ssq_stft_execute(ssq_stft_plan* pl, const void* x, int64_t batch, void* Sx, void* dSx,
                                void* Tx, void* w, void* stream) {
    SSQ_REQUIRE(pl && x && Sx, "ssq_stft_execute: null pointer");
    SSQ_REQUIRE(batch >= 1 && batch <= pl->d.max_batch, "batch %lld outside [1, %lld]",
                (long long)batch, (long long)pl->d.max_batch);
    SSQ_REQUIRE(!(Tx || w) || pl->have_ssq, "Tx / w requested but ssq parameters were not set");
    hipStream_t st = as_stream(stream);
    pl->order.enter(st);
    const int rc = dispatch_dtype(pl->d.dtype, [&](auto t) {
        return stft_execute_t<decltype(t)>(pl, x, batch, Sx, dSx, Tx, w, st);
    });
    pl->executed = true;
    pl->order.leave(st);
    return rc;
}

// the padded positions that copy signal sample j, per j (ascending): the transpose of the plan's signal extension
static int stft_adjoint_pad_table(ssq_stft_plan* pl) {
    if (pl->adj_off) return 0;
    const int64_t n = pl->d.n, m = pl->padlen, n1 = pl->n1;
    SSQ_REQUIRE(m < ((int64_t)1 << 31), "stft adjoint: padded length %lld", (long long)m);
    std::vector<int32_t> off, idx;                         // (the rule of pad_kernel / stft_pad_source)
    inverse_pad_table(n, m, n1, pl->d.padtype, off, idx);
    // (a failure part-way is undone by ssq_stft_adjoint)
    idx.push_back(0);                                      // (one entry of slack, as the table always had)
    int rc = pl->mem.upload(&pl->adj_idx, idx.data(), idx.size() * 4);
    if (!rc) rc = pl->mem.upload(&pl->adj_off, off.data(), off.size() * 4);
    return rc;
}

template <typename T>
static int stft_adjoint_unpad(ssq_stft_plan* pl, const void* ws, void* gx, int64_t batch, int64_t n_items,
                              int64_t step, int64_t span, int64_t pmax, hipStream_t stream) {
    dim3 grid((unsigned)((pl->d.n + 255) / 256), (unsigned)batch);
    hipLaunchKernelGGL((stft_adjoint_unpad_kernel<T>), grid, dim3(256), 0, stream, (const T*)ws, (T*)gx,
                       (const int32_t*)pl->adj_off, (const int32_t*)pl->adj_idx, pl->d.n, n_items, step, span, pmax);
    SSQ_LAUNCH_CHECK();
    return 0;
}

// the items of stft_adjoint_fused_kernel: frames per item -- what the strip holds, in whole passes of FP frames, fewer
// where that leaves the chip short of workgroups --, the items of a signal and the strip's length
static int stft_adjoint_items(StftAdjArgs& A, int L, int FP, int64_t batch) {
    const int hop = A.hop;
    int64_t nf = (ADJ_SPAN - L) / hop + 1;
    if (nf >= FP) {
        nf = nf / FP * FP;
        const int64_t want = ((A.n_hops * batch + 1023) / 1024 + FP - 1) / FP * FP;
        nf = std::max<int64_t>(FP, std::min(nf, want));
    }
    nf = std::min(nf, A.n_hops);
    A.nf = (int)nf;
    A.n_items = (A.n_hops + nf - 1) / nf;
    A.span = (int)((nf - 1) * hop + L);
    SSQ_REQUIRE(A.span <= ADJ_SPAN, "stft adjoint: strip of %d samples", A.span);
    return 0;
}

static int stft_adjoint_fused(ssq_stft_plan* pl, const void* gSx, const void* gdSx, void* gx, int64_t batch,
                              hipStream_t stream) {
    const ssq_stft_desc& d = pl->d;
    const int L = (int)d.n_fft, G = D_POINTS / L, hop = (int)d.hop_len;
    StftAdjArgs A;
    const bool both = gSx && gdSx;
    A.gA = (const float2*)(gSx ? gSx : gdSx); A.gB = both ? (const float2*)gdSx : nullptr;
    A.winA = (const float*)(gSx ? pl->window : pl->diff_window); A.winB = (const float*)pl->diff_window;
    A.ftw = (const c32*)pl->ftw;
    A.n_hops = pl->n_hops; A.rows = pl->rows; A.hop = hop; A.modulated = d.modulated; A.batch = (int)batch;
    int rc = stft_adjoint_items(A, L, both ? G : 2 * G, batch);
    if (rc) return rc;
    const int64_t nf = A.nf;
    StreamScratch scratch(stream);
    float* ws = nullptr;
    rc = scratch.alloc(&ws, (size_t)batch * A.n_items * A.span * sizeof(float));
    if (rc) return rc;
    A.ws = ws;
    rc = fft_dispatch<128, 2048>(L, [&](auto len) { return launch_stft_adjoint_fused<decltype(len)::value>(A, stream); });
    if (!rc) rc = stft_adjoint_unpad<float>(pl, ws, gx, batch, A.n_items, nf * hop, A.span,
                                            (pl->n_hops - 1) * (int64_t)hop + L, stream);
    return rc;
}

extern "C" int ssq_stft_adjoint(ssq_stft_plan* pl, const void* gSx, const void* gdSx, void* gx, int64_t batch,
                                void* stream) {
    SSQ_REQUIRE(pl && gx && (gSx || gdSx), "ssq_stft_adjoint: null pointer");
    SSQ_REQUIRE(batch >= 1 && batch <= pl->d.max_batch, "batch %lld outside [1, %lld]",
                (long long)batch, (long long)pl->d.max_batch);
    SSQ_REQUIRE(batch <= 65535, "ssq_stft_adjoint: batch %lld > 65535", (long long)batch);
    SSQ_REQUIRE(!gdSx || pl->diff_window, "the gradient of dSx needs a diff_window");
    hipStream_t st = as_stream(stream);
    pl->order.enter(st);
    const bool first = !pl->adj_off;
    const size_t before = pl->mem.count();
    int rc = stft_adjoint_pad_table(pl);
    if (!rc) {
        const ssq_stft_desc& d = pl->d;
        // (SSQ_DEBUG_STFT_ADJOINT_COMPOSED: the composed route on a fused plan, for comparisons)
        const bool fused = pl->fused && !getenv("SSQ_DEBUG_STFT_ADJOINT_COMPOSED") && d.hop_len < ((int64_t)1 << 24);
        if (fused) rc = stft_adjoint_fused(pl, gSx, gdSx, gx, batch, st);
        else {
            // composed: the overlap-added frames of the whole batch in the plan's padded-signal workspace, one strip
            rc = stft_adjoint_composed(d.dtype, gSx, gdSx, pl->window, pl->diff_window, pl->xp, batch, d.n_fft,
                                       pl->n_hops, d.hop_len, pl->padlen, d.modulated, st);
            if (!rc) rc = dispatch_dtype(d.dtype, [&](auto t) {
                return stft_adjoint_unpad<decltype(t)>(pl, pl->xp, gx, batch, 1, pl->padlen, pl->padlen, pl->padlen, st);
            });
        }
    }
    if (rc && first) {       // a first call that fails leaves the plan as it found it: the next one starts over
        pl->mem.release(before);
        pl->adj_off = pl->adj_idx = nullptr;
    }
    pl->order.leave(st);
    return rc;
}


// ---- inverse STFT (ssq_istft_batch / ssq_istft_adjoint of ssq_inverse.hip): the fused routes and the composed backward
namespace ssq {

// e^{2 pi i q / L} for the fused transforms, one table per (device, L), made at first use
static std::mutex g_tw_mu;
static std::map<std::pair<int, int>, void*> g_tw;
static int fused_twiddles(int L, const c32** out) {
    int dev = 0;
    SSQ_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tw_mu);
    auto it = g_tw.find({dev, L});
    if (it == g_tw.end()) {
        std::vector<float> tw;
        fft_twiddles(L, tw);
        void* d = nullptr;
        SSQ_CHECK_HIP(hipMalloc(&d, tw.size() * 4));
        SSQ_CHECK_HIP(hipMemcpy(d, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
        it = g_tw.emplace(std::make_pair(dev, L), d).first;
    }
    *out = (const c32*)it->second;
    return 0;
}

int istft_fused(const void* Sx, const void* win_t, const double* wn, void* x, int64_t batch, int64_t n_fft,
                int64_t n_hops, int64_t hop, int64_t N, int modulated, hipStream_t stream) {
    const int L = (int)n_fft, G = D_POINTS / L;
    StftAdjArgs A;
    A.gA = (const float2*)Sx; A.gB = nullptr; A.winA = (const float*)win_t; A.winB = nullptr;
    int rc = fused_twiddles(L, &A.ftw);
    if (rc) return rc;
    A.n_hops = n_hops; A.rows = L / 2 + 1; A.hop = (int)hop; A.modulated = modulated; A.batch = (int)batch;
    // (the items are sized as for one signal: a signal's sums then associate the same way in every batch, so that
    // slice b of a batched result has the bits of the single call)
    rc = stft_adjoint_items(A, L, 2 * G, 1);
    if (rc) return rc;
    StreamScratch scratch(stream);
    float* ws = nullptr;
    rc = scratch.alloc(&ws, (size_t)batch * A.n_items * A.span * sizeof(float));
    if (rc) return rc;
    A.ws = ws;
    rc = fft_dispatch<128, 2048>(L, [&](auto len) { return launch_stft_adjoint_fused<decltype(len)::value, true>(A, stream); });
    if (!rc) {
        hipLaunchKernelGGL(istft_finish_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)batch), dim3(256), 0, stream,
                           (const float*)ws, wn, (float*)x, N, (int64_t)(L / 2), A.n_items, (int64_t)A.nf * hop,
                           (int64_t)A.span, (n_hops - 1) * hop + L, 1.17549435e-38f);
        if (hipGetLastError() != hipSuccess) { set_error("istft_finish launch failed"); rc = -3; }
    }
    return rc;
}

int istft_adjoint_fused(const void* u, const void* win_t, void* gSx, int64_t batch, int64_t n_fft, int64_t n_hops,
                        int64_t hop, int64_t N, int modulated, hipStream_t stream) {
    const int L = (int)n_fft;
    StftFusedArgs A{};
    int rc = fused_twiddles(L, &A.ftw);
    if (rc) return rc;
    // the forward kernel over u, zero-extended by L / 2 on the left (the inverse's trim), window^a, no derivative
    A.window = (const float*)win_t; A.Sx = (float2*)gSx;
    A.padlen = N + L - 1; A.n_hops = n_hops; A.rows = L / 2 + 1;
    A.hop = (int)hop; A.s20 = L / 2; A.s21 = L / 2; A.modulated = modulated;
    A.x = (const float*)u; A.n = (int)N; A.n1 = L / 2; A.padtype = SSQ_PAD_ZERO;
    SsqParams sp{};
    return fft_dispatch<128, 2048>(L, [&](auto len) { return launch_stft_fused<decltype(len)::value, true>(A, sp, batch, stream); });
}

// gS[f][c] *= c_f / n_fft; the imaginary parts of DC and (even n_fft) Nyquist are exact zeros
template <typename T>
__global__ __launch_bounds__(256) void irfft_adjoint_weights_kernel(T* __restrict__ gS, int64_t rows, int64_t n_hops,
                                                                    int even, T inv_n) {
    const int64_t total = rows * n_hops;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = t / n_hops;
        const bool edge = f == 0 || (even && f == rows - 1);
        const T c = edge ? inv_n : T(2) * inv_n;
        gS[2 * t] = gS[2 * t] * c;
        gS[2 * t + 1] = edge ? T(0) : gS[2 * t + 1] * c;
    }
}

static StreamPlanCache<FftPlan> g_iadj_plans;             // R2C with transposed output; one work buffer per stream

template <typename T>
static int istft_adjoint_composed_t(int dtype, const void* upad, const void* win_t, void* gSx, int64_t batch,
                                    int64_t n_fft, int64_t n_hops, int64_t hop, int64_t ulen, int modulated,
                                    hipStream_t stream) {
    const int64_t rows = n_fft / 2 + 1, total = n_fft * n_hops;
    const int64_t s20 = (n_fft + 1) / 2, s21 = n_fft / 2;
    StreamScratch scratch(stream);
    T* frames = nullptr;
    int rc = scratch.alloc(&frames, (size_t)total * sizeof(T));
    if (rc) return rc;
    const unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    const unsigned g2 = (unsigned)std::min<int64_t>((rows * n_hops + 255) / 256, 8192);
    for (int64_t b = 0; b < batch && !rc; ++b) {
        hipLaunchKernelGGL((frame_window_kernel<T>), dim3(g), dim3(256), 0, stream, (const T*)upad + (size_t)b * ulen,
                           (const T*)win_t, (const T*)nullptr, frames, (T*)nullptr, n_fft, n_hops, hop, s20, s21, modulated);
        if (hipGetLastError() != hipSuccess) { set_error("frame_window launch failed"); rc = -3; break; }
        T* out = (T*)gSx + (size_t)b * rows * n_hops * 2;
        {
            std::lock_guard<std::mutex> lock(g_iadj_plans.mu);    // held until the transform is enqueued
            FftPlan* f = nullptr;
            rc = g_iadj_plans.get(dtype, n_fft, n_hops, stream, &f, [&](FftPlan& p) {
                return p.create(0, dtype, (size_t)n_fft, (size_t)n_hops, 1.0, (size_t)n_fft, 1, (size_t)n_hops);
            });
            if (!rc) rc = f->execute(frames, out, stream);
        }
        if (rc) break;
        hipLaunchKernelGGL((irfft_adjoint_weights_kernel<T>), dim3(g2), dim3(256), 0, stream, out, rows, n_hops,
                           (int)(n_fft % 2 == 0), (T)(T(1) / (T)n_fft));
        if (hipGetLastError() != hipSuccess) { set_error("irfft_adjoint_weights launch failed"); rc = -3; }
    }
    return rc;
}

int istft_adjoint_composed(int dtype, const void* upad, const void* win_t, void* gSx, int64_t batch, int64_t n_fft,
                           int64_t n_hops, int64_t hop, int64_t ulen, int modulated, hipStream_t stream) {
    return dispatch_dtype(dtype, [&](auto t) {
        return istft_adjoint_composed_t<decltype(t)>(dtype, upad, win_t, gSx, batch, n_fft, n_hops, hop, ulen, modulated,
                                                     stream);
    });
}

}  // namespace ssq
