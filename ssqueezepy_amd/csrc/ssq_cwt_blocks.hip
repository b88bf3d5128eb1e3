// ssq_cwt_blocks.hip -- the block rows of the CWT: an overlap-save "zoom" inverse FFT that stays in LDS, fused with
// the unpad / phase-transform / bin-map epilogue. gfx950.
//
// Math (see ssqueezepy_amd/_blocks.py for the derivation and the host planning):
// a row whose impulse response fits +-m samples is evaluated block by block; block b
// of class (P, m, V) covers padded samples t0 = n1 - m + b*V ... t0 + P and is exact
// on its central V samples. With X_b = FFT_P(block) and the wavelet's P-grid samples
// psi[kappa] (the M-grid bank at every (M/P)-th bin), block output sample
//   t = q*R' + c   (R' = P/L', q in [0, L'), c in [0, R'))
// is   y[t] = sum_kappa  psi[kappa] X_b[kappa] e^{2i pi kappa c / P} / P  *  e^{2i pi kappa q / L'}
// i.e. entry q of an L'-point inverse FFT whose input at (kappa mod L') is the band
// entry times a per-column twiddle. The derivative row uses inputs times 1j*xi/dt.
//
// One float32 workgroup (256 threads) is one (row, block, group of G adjacent columns): L' G = 4096 complex points,
// 16 per thread, laid out in LDS as [q][g] with the column index fastest. Its outputs stay in registers and go to HBM
// as runs of G adjacent time samples: Wx (8 B per point) and the bin map (2 B per point) are written once, the inputs
// (the band of X_b, psi, twiddles: a few KiB per workgroup) come from L2, and no intermediate array is written.
//
// The unit holds, in this order:
//   ssq_block_emit.inl     the per-point pieces of the fused epilogue, shared by the zoom kernels and the exact rows;
//   the float32 zoom kernels: a prologue (column twiddles staged in LDS, the band in one of three forms), the transform
//                          (lds_ifft2 for Wx and dWx as a pair, lds_ifft for one plane) and the epilogue, in seven
//                          builds (`ZoomLean` ...), per class (blockzoom_kernel) or all classes (blockzoom_multi_kernel);
//   the float64 zoom kernel, with a body of its own, and BlockPlan::run64;
//   ssq_block_spectra.inl  the block spectra X_b (gather + rocFFT, or the library's own kernels), BlockPlan::spectra;
//   BlockPlan::create, destroy, bytes and run;
//   ssq_block_exact.inl    the four-step exact rows: ExactArgs, the two pass kernels, setup_exact and run_exact.
//
// Compiled with -ffp-contract=off because the epilogue computes bin indices with the
// exact operation sequence of the CPU path (ssq_point_math.inl); the FFT butterflies
// use explicit fmaf.
#include "ssq_common.h"
#include "ssq_blocks.h"
#include "ssq_ldsfft.h"
#include <cmath>

namespace ssq {

#include "ssq_point_math.inl"
#include "ssq_block_emit.inl"

struct BlockArgs {
    const int4* items;                 // (row, block, c0, class)
    const BlockRowDev* rows;
    const BlockClassDev* classes;
    const float* pbank;
    const float* pxi;
    const c32* ctw;                    // per-class column twiddles e^{2 pi i q / P}
    const c32* ftw;                    // e^{2 pi i q / L}
    const c32* xb;                     // block spectra, all classes, all signals
    const float* row_scale;
    float* Wx; float* dWx; float* w; unsigned short* kidx;
    int64_t M, N, na, n_items;
    double h;                          // 2 pi / M
    float inv_dt;
    double gamma;
    int sig;                           // first signal of the launch (blockIdx.y adds to it)
    // which build a call takes: the fused ssq_cwt form (Wx + bin map, unscaled), Wx alone (a plain cwt)
    bool lean() const { return kidx && !dWx && !w && !row_scale; }
    bool wx_alone() const { return !kidx && !dWx && !w; }
};

// ---- the seven builds of the float32 zoom kernels: tag types, and what each implies
//   LEAN:   the fused ssq_cwt form, Wx + bin map only, with an epilogue of its own (emit_point);
//   NOD:    a plain cwt (no dWx, no w, no bin map): the derivative is compiled out (config 1's block rows 27 -> 17 us);
//   PAIRED: Wx and dWx go through each LDS pass as a pair (lds_ifft2; block rows 57.1 -> 51.1 us at config 2,
//           profiles/block_paired_passes.txt); false: one transform after the other;
//   BAND:   the band is staged once per workgroup in the paired transform's buffer; false: outside it.
// The BandOut builds (SSQ_DEBUG_BLOCK_BAND=0) and the Unpaired ones (SSQ_DEBUG_BLOCK_PAIRED=0) make the bits of
// ZoomLean / ZoomFull the earlier way: they are what the tests compare those two with.
template <bool LEAN_, bool NOD_, bool PAIRED_, bool BAND_> struct ZoomFlags {
    static constexpr bool LEAN = LEAN_, NOD = NOD_, PAIRED = PAIRED_, BAND = BAND_;
    static_assert((!BAND || PAIRED) && (!NOD || (!LEAN && !PAIRED)), "the band sits in the paired transform's buffer; Wx alone has one plane");
};
struct ZoomWxAlone      : ZoomFlags<false, true, false, false> {};
struct ZoomLean         : ZoomFlags<true, false, true, true> {};
struct ZoomLeanBandOut  : ZoomFlags<true, false, true, false> {};
struct ZoomLeanUnpaired : ZoomFlags<true, false, false, false> {};
struct ZoomFull         : ZoomFlags<false, false, true, true> {};
struct ZoomFullBandOut  : ZoomFlags<false, false, true, false> {};
struct ZoomFullUnpaired : ZoomFlags<false, false, false, false> {};
// host: f(the build) for what a call asks for (BlockArgs::wx_alone, lean) and the plan's two switches; returns f's status
template <typename F>
static int dispatch_zoom_build(bool wx_alone, bool lean, bool paired, bool band, F&& f) {
    if (wx_alone) return f(ZoomWxAlone{});
    if (lean) return paired && band ? f(ZoomLean{}) : paired ? f(ZoomLeanBandOut{}) : f(ZoomLeanUnpaired{});
    return paired && band ? f(ZoomFull{}) : paired ? f(ZoomFullBandOut{}) : f(ZoomFullUnpaired{});
}

struct __align__(16) BandRec { c32 b; float mm, pad; };     // psi X / P and pxi / dt of one band element: one 16-byte LDS access
// The body of one workgroup (item `item_idx` of the class's list; blockIdx.y = signal of the launch). Its LDS
// arrays come from the caller: blockzoom_kernel sizes them for its class, blockzoom_multi_kernel -- every class
// in ONE launch, for transforms too small to fill the GPU per class -- shares one set between the classes.
template <int L, typename Z>
__device__ __forceinline__ void blockzoom_body(const BlockArgs& A, const SsqParams& sp, int item_idx,
                                               c32* __restrict__ buf, c32* __restrict__ spow,
                                               c32* __restrict__ wrapf, c32* __restrict__ bandW,
                                               c32* __restrict__ bandD) {
    using S = FftShape<L>;
    constexpr int G = S::G, R1 = S::R1, RL = S::RL;      // (RL: the last radix)
    constexpr bool LEAN = Z::LEAN, NOD = Z::NOD, PAIRED = Z::PAIRED, BAND = Z::BAND;
    const int tid = threadIdx.x;
    const int4 item = A.items[item_idx];
    const int row = item.x, blk = item.y, c0 = item.z;
    const BlockRowDev r = A.rows[row];
    const BlockClassDev cl = A.classes[item.w];
    const int P = (int)cl.P, Rp = P / L;
    const int sig = A.sig + (int)blockIdx.y;
    const c32* xb = A.xb + cl.xb_off + ((int64_t)sig * cl.nb + blk) * cl.xb_stride;
    const c32* ctw = A.ctw + cl.ctw_off;
    const float* psi = A.pbank + r.pb_off;
    const float* pxi = A.pxi + r.pb_off;

    // ---- prologue: pass-1 inputs of both transforms, in registers.
    // Input slot q of column c holds  psi[kap] X[kap] e^{2 pi i kap c / P} / P  with
    // kap = klo + ((q - klo) mod L). A thread's R1 slots are q = u + t*STR, so its bins
    // advance by STR (minus L on wrap-around): the column twiddle is one table gather
    // for t = 0 times a power of s_c = e^{2 pi i STR c / P} (and the wrap factor
    // e^{-2 pi i L c / P}), and those powers -- R1 x G values per workgroup -- are staged
    // in LDS once (spow: R1 * G entries, wrapf: G). 8x fewer scattered table gathers than one per point (the
    // gathers, not the arithmetic, bounded this stage).
    // The band (psi X / P and its derivative multiple) is the same for all G columns of the workgroup. Three forms:
    //   LDS (L' <= 512): formed once per workgroup in bW / bD, L' entries each -- bandW / bandD, or with BAND the
    //     first 2 L' entries of `buf`, idle until pass 1's first store (lds_ifft2<L, false> takes a barrier there).
    //   RECORDS (L' >= 1024 with BAND): a work-item loads L' / 256 band elements at consecutive addresses, forms
    //     psi X / P and pxi / dt once per element and stores them in `buf` as a 16-byte record at the element's FFT
    //     slot (klo + off) mod L'; behind the barrier it reads its 16 records at u + k STR, conflict-free (consecutive
    //     lanes: consecutive records, a group's G lanes the same one). The products are those of the next form.
    //   REGISTERS (L' >= 1024 without BAND: Wx alone and the comparator builds): three global loads per point.
    // The two forms for L' >= 1024 issue every global load of the prologue up front, into registers, and only then
    // write the staged values to LDS and take the barrier: the band's latency runs under the staging (block rows
    // 69.4 -> 64.0 us; an ablation without the band's loads runs at 51.8: profiles/r5_ab_history.txt).
    constexpr bool STAGE = (L <= 512);
    constexpr bool BAND_REC = BAND && !STAGE;
    static_assert(STAGE || R1 * G <= NT, "blockzoom_body: L' >= 1024 stages one twiddle per work-item, loaded ahead of the barrier");
    static_assert(sizeof(BandRec) == 2 * sizeof(c32) && 2 * L <= lds_ifft2_points<L>, "either form of the band: 2 L' entries of buf");
    BandRec* __restrict__ const rec = reinterpret_cast<BandRec*>(buf);
    c32* const bW = BAND ? buf : bandW;
    c32* const bD = BAND ? buf + L : bandD;
    const float invP = 1.0f / (float)P;             // exact (P is a power of two)
    constexpr int NREG = (STAGE || BAND_REC) ? 1 : PPT;          // (REGISTERS: the band's loads per point)
    float e_p[NREG], e_m[NREG];
    c32 e_X[NREG], e_cw[STAGE ? 1 : PPT / R1];
    if constexpr (!STAGE) {
        constexpr int NBe = PPT / R1, STR = L / R1;
        c32 st_v = {0.f, 0.f}, st_w = {0.f, 0.f};
        if (tid < R1 * G) {
            const unsigned t = (unsigned)(tid / G), col = (unsigned)(c0 + tid % G);
            st_v = ctw[(t * (unsigned)STR * col) & (unsigned)(P - 1)];
        }
        if (tid < G) st_w = ctw[(0u - (unsigned)L * (unsigned)(c0 + tid)) & (unsigned)(P - 1)];
#pragma unroll
        for (int it = 0; it < NBe; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
            const int off0 = (u - r.klo) & (L - 1);
            e_cw[it] = ctw[((unsigned)(r.klo + off0) * (unsigned)(c0 + g)) & (unsigned)(P - 1)];
            if constexpr (!BAND_REC) {
#pragma unroll
                for (int k = 0; k < R1; ++k) {
                    const int off = (off0 + k * STR) & (L - 1);
                    const bool in = off < r.KP;              // slots past the band: zeros
                    e_p[it * R1 + k] = in ? psi[off] : 0.f;
                    e_X[it * R1 + k] = in ? xb[r.klo + off] : c32{0.f, 0.f};
                    e_m[it * R1 + k] = in ? pxi[off] : 0.f;
                }
            }
        }
        if constexpr (BAND_REC) {
            constexpr int NE = L / NT;
            float s_p[NE], s_m[NE]; c32 s_X[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int off = tid + i * NT;
                const bool in = off < r.KP;                  // slots past the band: zeros, through the same products
                s_p[i] = in ? psi[off] : 0.f;
                s_X[i] = in ? xb[r.klo + off] : c32{0.f, 0.f};
                s_m[i] = in ? pxi[off] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const float p = s_p[i] * invP;
                BandRec b;
                b.b = {p * s_X[i].x, p * s_X[i].y};
                b.mm = s_m[i] * A.inv_dt;
                b.pad = 0.f;
                rec[(r.klo + tid + i * NT) & (L - 1)] = b;
            }
        }
        if (tid < R1 * G) spow[tid] = st_v;
        if (tid < G) wrapf[tid] = st_w;
    } else {
        constexpr int STR = L / R1;
        for (int i = tid; i < R1 * G; i += NT) {
            const unsigned t = (unsigned)(i / G), col = (unsigned)(c0 + i % G);
            spow[i] = ctw[(t * (unsigned)STR * col) & (unsigned)(P - 1)];
        }
        if (tid < G) {
            const unsigned col = (unsigned)(c0 + tid);
            wrapf[tid] = ctw[(0u - (unsigned)L * col) & (unsigned)(P - 1)];
        }
        for (int off = tid; off < L; off += NT) {
            c32 b = {0.f, 0.f}, d = {0.f, 0.f};
            if (off < r.KP) {
                const float p = psi[off] * invP;
                const c32 X = xb[r.klo + off];
                b = {p * X.x, p * X.y};
                const float mm = pxi[off] * A.inv_dt;   // 1j*xi/dt, xi as the reference stores it
                d = {-(b.y * mm), b.x * mm};
            }
            bW[off] = b; bD[off] = d;
        }
    }
    __syncthreads();
    c32 zw[PPT], zd[PPT];
    {
        constexpr int NB = PPT / R1, STR = L / R1;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
            const unsigned col = (unsigned)(c0 + g);
            const int off0 = (u - r.klo) & (L - 1);
            c32 cw0;
            if constexpr (STAGE) cw0 = ctw[((unsigned)(r.klo + off0) * col) & (unsigned)(P - 1)];
            else cw0 = e_cw[it];
            const c32 wf = wrapf[g];
#pragma unroll
            for (int k = 0; k < R1; ++k) {
                const int offu = off0 + k * STR;            // < 2L
                const int off = offu & (L - 1);             // band element at FFT slot q
                c32 z = {0.f, 0.f}, dz = {0.f, 0.f};
                if constexpr (STAGE) {
                    c32 cw = (k == 0) ? cw0 : cmul_v(cw0, spow[k * G + g]);
                    if (offu >= L) cw = cmul_v(cw, wf);
                    z = cmul_v(bW[off], cw);
                    dz = cmul_v(bD[off], cw);
                } else if constexpr (BAND_REC) {
                    const BandRec br = rec[u + k * STR];     // FFT slot q = u + k STR holds band element `off`
                    c32 cw = (k == 0) ? cw0 : cmul_v(cw0, spow[k * G + g]);
                    if (offu >= L) cw = cmul_v(cw, wf);
                    z = cmul_v(br.b, cw);
                    dz = {-(z.y * br.mm), z.x * br.mm};
                } else {
                    const float p = e_p[it * R1 + k] * invP;
                    const c32 X = e_X[it * R1 + k];
                    c32 cw = (k == 0) ? cw0 : cmul_v(cw0, spow[k * G + g]);
                    if (offu >= L) cw = cmul_v(cw, wf);
                    const c32 bz = {p * X.x, p * X.y};
                    z = cmul_v(bz, cw);
                    const float mm = e_m[it * R1 + k] * A.inv_dt;
                    dz = {-(z.y * mm), z.x * mm};
                }
                zw[it * R1 + k] = z; zd[it * R1 + k] = dz;
            }
        }
    }
    // (twiddles requested ahead of each pass' barrier; nothing has touched `buf` before the first transform:
    // 58.9 -> 56.7 -> 56.2 us at config 2, round 5)
    // (... with BAND it holds the band, and the paired transform waits for every wavefront's reads of it)
    if constexpr (PAIRED) {
        lds_ifft2<L, !BAND>(zw, zd, buf, A.ftw, tid);
    } else {
        lds_ifft<L, true, true>(zw, buf, A.ftw, tid);
        if constexpr (!NOD) lds_ifft<L, true>(zd, buf, A.ftw, tid);
    }

    // ---- epilogue: unpad, store, phase transform, bin map (written out here and in exact_pass2_kernel: through one
    // function with the column map as a functor both come out as other code, profiles/block_rows_refactor_isa.txt)
    constexpr int NB = PPT / RL, STR = L / RL;
    const EmitRow er = make_emit_row(A.Wx, A.dWx, A.w, A.kidx, A.row_scale, sig, (int)blockIdx.y, row, A.na, A.N, A.gamma, sp.flipud);
    const int m = (int)cl.m, N = (int)A.N;
    const int jbase = blk * (int)cl.V - m + c0;
    // valid outputs of the block: samples [m, m + V) that fall inside the signal
    const unsigned span = (unsigned)max(0, min((int)cl.V, N - blk * (int)cl.V));
    unsigned pend = 0;                              // slots whose bin needs the exact map
    auto emit_all = [&](auto grid_tag) {
        constexpr int GRID = decltype(grid_tag)::value;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < RL; ++k) {
                const int dcol = (u + k * STR) * Rp + g + (c0 - m);   // sample index inside the block - margin
                if ((unsigned)dcol >= span) continue;               // margin or past the signal's end
                const int j = dcol + blk * (int)cl.V;               // output column
                if constexpr (NOD) {                                 // Wx alone (rs == 1, exact, when unscaled)
                    er.W[j] = make_float2(zw[it * RL + k].x * er.rs, zw[it * RL + k].y * er.rs);
                    continue;
                }
                if (emit_point<LEAN, GRID>(er, j, zw[it * RL + k], NOD ? c32{0.f, 0.f} : zd[it * RL + k], sp))
                    pend |= 1u << (it * RL + k);
            }
        }
    };
    dispatch_grid<LEAN>(sp.grid, emit_all);
    // rare: points inside a screen's guard band. One pending point per lane and round,
    // picked with compile-time slot indices (zw/zd stay in registers).
    while (__builtin_amdgcn_ballot_w64(pend != 0)) {
        const unsigned low = pend & (0u - pend);
        pend ^= low;
        c32 W = {0.f, 0.f}, D = {0.f, 0.f};
        int j = 0;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < RL; ++k)
                if (low == (1u << (it * RL + k))) {
                    W = zw[it * RL + k]; D = NOD ? c32{0.f, 0.f} : zd[it * RL + k]; j = jbase + (u + k * STR) * Rp + g;
                }
        }
        if (low) emit_point_exact(er, er.k + j, W, D, sp);
    }
}

template <int L, typename Z>
__global__ __launch_bounds__(NT) void blockzoom_kernel(BlockArgs A, SsqParams sp) {
    __shared__ __align__(16) c32 buf[Z::PAIRED ? lds_ifft2_points<L> : D_POINTS];
    __shared__ c32 spow[FftShape<L>::R1 * FftShape<L>::G];
    __shared__ c32 wrapf[FftShape<L>::G];
    __shared__ c32 bandW[(L <= 512 && !Z::BAND) ? L : 1], bandD[(L <= 512 && !Z::BAND) ? L : 1];
    blockzoom_body<L, Z>(A, sp, (int)blockIdx.x, buf, spow, wrapf, bandW, bandD);
}

// every class of a plan in one launch: workgroup b belongs to the class whose item range holds b
struct BlockMultiArgs {
    BlockArgs A;                       // (items, n_items, ftw: filled per class inside)
    const int4* items[5]; const c32* ftw[5];
    int first[6];                      // first workgroup of class s; first[5] = grid size
};
// With the band inside `buf` four workgroups fit a CU's 160 KiB of LDS (4 x 39 168 B). The lean build is held to the 128
// registers that four wavefronts per SIMD leave each of them (left alone it takes 138, which is three): block rows
// 51.2 -> 46.7 us at config 2, every run below every run of the parent (profiles/block_band_staged.txt; at three
// workgroups per CU the staged band alone does not separate from the parent). 20 registers spill. The other builds stay
// as the compiler sizes them (the full build would spill 65).
template <typename Z>
__global__ __launch_bounds__(NT) SSQ_WAVES_PER_EU((Z::LEAN && Z::BAND) ? 4 : 1, (Z::LEAN && Z::BAND) ? 4 : 8)
void blockzoom_multi_kernel(BlockMultiArgs M, SsqParams sp) {
    __shared__ __align__(16) c32 buf[Z::PAIRED ? lds_ifft2_points<2048> : D_POINTS];      // (the padded buffer: the same for every L' that pads)
    __shared__ c32 spow[512];          // max R1 * G (16 x 32)
    __shared__ c32 wrapf[32];
    __shared__ c32 bandW[Z::BAND ? 1 : 512], bandD[Z::BAND ? 1 : 512];   // (BAND: inside buf -- 39 KB of LDS instead of 47)
    const int b = (int)blockIdx.x;
    int s = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k) s += b >= M.first[k];
    BlockArgs A = M.A;
    A.items = M.items[s]; A.ftw = M.ftw[s];
    const int it = b - M.first[s];
    // (written out: through fft_switch's lambda the compiler lays this kernel out differently from the code that was measured)
    switch (s) {
        case 0: blockzoom_body<128, Z>(A, sp, it, buf, spow, wrapf, bandW, bandD); break;
        case 1: blockzoom_body<256, Z>(A, sp, it, buf, spow, wrapf, bandW, bandD); break;
        case 2: blockzoom_body<512, Z>(A, sp, it, buf, spow, wrapf, bandW, bandD); break;
        case 3: blockzoom_body<1024, Z>(A, sp, it, buf, spow, wrapf, bandW, bandD); break;
        default: blockzoom_body<2048, Z>(A, sp, it, buf, spow, wrapf, bandW, bandD); break;
    }
}

// ======================================================================= float64 block rows
// The same block decomposition in double precision: 2048 points per 128-thread workgroup
// (32 KiB of LDS, 16 points per thread), twiddles and spectra in double, the exact
// (double) bin map for every point. No lean variant, no LDS band staging.
struct BlockArgs64 {
    const int4* items; const BlockRowDev* rows; const BlockClassDev* classes;
    const double* pbank; const double* pxi;
    const c64* ctw; const c64* ftw; const c64* xb;
    const double* row_scale;
    double* Wx; double* dWx; double* w; unsigned short* kidx;
    int64_t M, N, na, n_items;
    double inv_dt, gamma;
    int sig;
    bool wx_alone() const { return !kidx && !dWx && !w; }
};

// (two wavefronts per SIMD: left alone the compiler takes 276-280 registers -- one wavefront per SIMD -- and config 5's
// block rows run at 10.5 ms instead of 8.1; at 256 it spills ~90 bytes per lane)
// NOD: Wx alone (a plain cwt), as for the float32 kernels: the derivative's transform and outputs compiled out.
template <int L, bool NOD = false>
__global__ __launch_bounds__(FftGeom<double>::NT) SSQ_WAVES_PER_EU(2, 2) void blockzoom_f64_kernel(BlockArgs64 A, SsqParams sp) {
    using S = FftShape<L, double>;
    constexpr int NT64 = FftGeom<double>::NT, G = S::G, R1 = S::R1, RL = S::RL;
    __shared__ c64 buf[FftGeom<double>::D];
    __shared__ c64 spow[R1 * G];
    __shared__ c64 wrapf[G];
    const int tid = threadIdx.x;
    const int4 item = A.items[blockIdx.x];
    const int row = item.x, blk = item.y, c0 = item.z;
    const BlockRowDev r = A.rows[row];
    const BlockClassDev cl = A.classes[item.w];
    const int P = (int)cl.P, Rp = P / L;
    const int sig = A.sig + (int)blockIdx.y;
    const c64* xb = A.xb + cl.xb_off + ((int64_t)sig * cl.nb + blk) * cl.xb_stride;
    const c64* ctw = A.ctw + cl.ctw_off;
    const double* psi = A.pbank + r.pb_off;
    const double* pxi = A.pxi + r.pb_off;
    const double invP = 1.0 / (double)P;
    // (round 6, as in the float32 kernels since round 5: the band's three loads per point are issued BEFORE the barrier
    // behind the staged twiddles -- two dependent round trips become one; config 5 "r6y21")
    constexpr int NBP = PPT / R1, STRP = L / R1;
    double bp[PPT], bm[PPT]; c64 bX[PPT];
#pragma unroll
    for (int it = 0; it < NBP; ++it) {
        const int u = (tid + it * NT64) / G;
        const int off0 = (u - r.klo) & (L - 1);
#pragma unroll
        for (int k = 0; k < R1; ++k) {
            const int off = (off0 + k * STRP) & (L - 1);
            const int oc = off < r.KP ? off : 0;             // unconditional, clamped loads
            bp[it * R1 + k] = psi[oc]; bX[it * R1 + k] = xb[r.klo + oc]; bm[it * R1 + k] = pxi[oc];
        }
    }
    {
        constexpr int STR = L / R1;
        for (int i = tid; i < R1 * G; i += NT64) {
            const unsigned t = (unsigned)(i / G), col = (unsigned)(c0 + i % G);
            spow[i] = ctw[(t * (unsigned)STR * col) & (unsigned)(P - 1)];
        }
        if (tid < G) {
            const unsigned col = (unsigned)(c0 + tid);
            wrapf[tid] = ctw[(0u - (unsigned)L * col) & (unsigned)(P - 1)];
        }
    }
    c64 cw0s[NBP];
#pragma unroll
    for (int it = 0; it < NBP; ++it) {
        const int idx = tid + it * NT64, g = idx % G, u = idx / G;
        const int off0 = (u - r.klo) & (L - 1);
        cw0s[it] = ctw[((unsigned)(r.klo + off0) * (unsigned)(c0 + g)) & (unsigned)(P - 1)];
    }
    __syncthreads();
    c64 zw[PPT], zd[PPT];
    {
        constexpr int NB = PPT / R1, STR = L / R1;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT64, g = idx % G, u = idx / G;
            const int off0 = (u - r.klo) & (L - 1);
            const c64 cw0 = cw0s[it];
            const c64 wf = wrapf[g];
#pragma unroll
            for (int k = 0; k < R1; ++k) {
                const int offu = off0 + k * STR, off = offu & (L - 1);
                const bool in = off < r.KP;
                const double p = bp[it * R1 + k] * invP;
                const c64 X = bX[it * R1 + k];
                const double mm = bm[it * R1 + k] * A.inv_dt;
                c64 cw = (k == 0) ? cw0 : cmul(cw0, spow[k * G + g]);
                if (offu >= L) cw = cmul_v(cw, wf);
                const c64 bz = {p * X.x, p * X.y};
                const c64 zz = cmul_v(bz, cw);
                c64 z = {0.0, 0.0}, dz = {0.0, 0.0};
                if (in) { z = zz; dz = {-(zz.y * mm), zz.x * mm}; }
                zw[it * R1 + k] = z; zd[it * R1 + k] = dz;
            }
        }
    }
    lds_ifft<L, false, true>(zw, buf, A.ftw, tid);      // (the buffer is untouched so far: no barrier in front)
    if constexpr (!NOD) lds_ifft<L>(zd, buf, A.ftw, tid);

    constexpr int NB = PPT / RL, STR = L / RL;
    const int64_t base = ((int64_t)sig * A.na + row) * A.N;
    double2* Wo = reinterpret_cast<double2*>(A.Wx) + base;
    double2* Do = A.dWx ? reinterpret_cast<double2*>(A.dWx) + base : nullptr;
    double* wo = A.w ? A.w + base : nullptr;
    unsigned short* ko = A.kidx ? A.kidx + ((int64_t)blockIdx.y * A.na + row) * A.N : nullptr;
    const double rs = A.row_scale ? A.row_scale[row] : 1.0;
    const int64_t omax = A.na - 1;
    const int m = (int)cl.m, N = (int)A.N;
    const unsigned span = (unsigned)max(0, min((int)cl.V, N - blk * (int)cl.V));
#pragma unroll
    for (int it = 0; it < NB; ++it) {
        const int idx = tid + it * NT64, g = idx % G, u = idx / G;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            const int dcol = (u + k * STR) * Rp + g + (c0 - m);
            if ((unsigned)dcol >= span) continue;
            const int j = dcol + blk * (int)cl.V;
            const c64 W = zw[it * RL + k], D = NOD ? c64{0.0, 0.0} : zd[it * RL + k];
            const double c = W.x * rs, d = W.y * rs, a = D.x * rs, b = D.y * rs;
            Wo[j] = make_double2(c, d);
            if constexpr (NOD) continue;
            if (Do) Do[j] = make_double2(a, b);
            if (wo) wo[j] = mag_lt(c, d, A.gamma) ? (double)INFINITY : fabs(phase_ratio(a, b, c, d));
            if (ko) {
                unsigned short kk = 0xFFFFu;
                if (mag_gt(c, d, A.gamma)) {
                    const int64_t kb = bin_of_point(a, b, c, d, false, 0.0, sp, omax);
                    kk = (unsigned short)(sp.flipud ? omax - kb : kb);
                }
                ko[j] = kk;
            }
        }
    }
}

template <int L>
static int launch_zoom64(const BlockArgs64& A, const SsqParams& sp, int nsig, hipStream_t stream) {
    if (A.n_items == 0) return 0;
    const dim3 grid((unsigned)A.n_items, (unsigned)nsig);
    return dispatch_bool(A.wx_alone(), [&](auto nod) {
        hipLaunchKernelGGL((blockzoom_f64_kernel<L, decltype(nod)::value>), grid, dim3(FftGeom<double>::NT), 0, stream, A, sp);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int BlockPlan::run64(int sig, int nsig, double* Wx, double* dWx, double* w, unsigned short* kidx,
                     const double* row_scale, double dt, const SsqParams& sp, hipStream_t stream) {
    BlockArgs64 A;
    A.rows = rows; A.classes = classes; A.pbank = (const double*)pbank; A.pxi = (const double*)pxi;
    A.ctw = (const c64*)ctw; A.xb = (const c64*)xb; A.row_scale = row_scale;
    A.Wx = Wx; A.dWx = dWx; A.w = w; A.kidx = kidx;
    A.M = M; A.N = N; A.na = na;
    A.inv_dt = 1.0 / dt; A.gamma = sp.gamma; A.sig = sig;
    for (int s = 0; s < 5; ++s) {                  // the plan's item lists: L' = 128 << s
        A.items = (const int4*)items[s]; A.n_items = n_items[s];
        A.ftw = (const c64*)ftw + ftw_off[s];
        const int rc = fft_dispatch<128, 2048>(128 << s, [&](auto len) { return launch_zoom64<decltype(len)::value>(A, sp, nsig, stream); });
        if (rc) return rc;
    }
    return 0;
}

#include "ssq_block_spectra.inl"

int BlockPlan::create(const ssq_cwt_blocks_desc& d, int dtype_, int64_t M_, int64_t N_, int64_t n1_,
                      int64_t na_, int64_t max_batch_) {
    M = M_; N = N_; n1 = n1_; na = na_; max_batch = max_batch_; dtype = dtype_;
    const size_t rs = dtype == SSQ_F32 ? 4 : 8;
    nc = d.n_classes;
    hcls.resize(nc);
    int64_t xb_total = 0, blk_max = 0;
    for (int c = 0; c < nc; ++c) {
        BlockClassDev& k = hcls[c];
        k.P = d.classes[5 * c]; k.m = d.classes[5 * c + 1]; k.V = d.classes[5 * c + 2];
        k.nb = d.classes[5 * c + 3];
        k.analytic = d.classes[5 * c + 4] ? 1 : 0;
        SSQ_REQUIRE(c == 0 || hcls[c - 1].analytic <= k.analytic, "block classes: analytic classes must come last");
        k.ctw_off = d.ctw_off[c];
        k.xb_stride = k.analytic ? k.P : k.P / 2 + 1;
        k.xb_off = xb_total;
        xb_total += max_batch * k.nb * k.xb_stride;
        k.blk_off = blk_max;
        if (!k.analytic) blk_max += max_batch * k.nb * k.P;
        n_analytic += (int)k.analytic;
    }
    int rc;
    if ((rc = mem.upload(&classes, hcls.data(), sizeof(BlockClassDev) * nc))) return rc;
    static_assert(sizeof(BlockRowDev) == 6 * sizeof(int32_t), "row table layout");
    if ((rc = mem.upload(&rows, d.rows, sizeof(BlockRowDev) * na))) return rc;
    if ((rc = mem.upload(&pbank, d.pbank, rs * d.n_pbank))) return rc;
    if ((rc = mem.upload(&pxi, d.pxi, rs * d.n_pbank))) return rc;
    if ((rc = mem.upload(&ctw, d.ctw, 2 * rs * (size_t)d.ctw_off[nc]))) return rc;
    if ((rc = mem.upload(&ftw, d.ftw, 2 * rs * (size_t)d.n_ftw))) return rc;
    for (int s = 0; s < 5; ++s) {
        n_items[s] = d.n_items[s];
        ftw_off[s] = d.ftw_off[s];
        if ((rc = mem.upload(&items[s], d.items[s], sizeof(int4) * (size_t)d.n_items[s]))) return rc;
        if (d.n_items[s]) h_items[s].assign(d.items[s], d.items[s] + 4 * d.n_items[s]);
    }
    if ((rc = mem.alloc(&xb, 2 * rs * (size_t)xb_total))) return rc;
    if ((rc = mem.alloc(&blocks, rs * (size_t)blk_max))) return rc;
    // classes of equal block length and kind are contiguous in `blocks` and `xb`: one batched
    // real-to-complex transform per length (complex, in place in `xb`, for the analytic classes)
    for (int c = 0; c < nc;) {
        int e = c;
        int64_t nblocks = 0;
        while (e < nc && hcls[e].P == hcls[c].P && hcls[e].analytic == hcls[c].analytic)
            nblocks += max_batch * hcls[e++].nb;
        FftPlan fp;
        rc = fp.create(hcls[c].analytic ? 2 : 0, dtype, (size_t)hcls[c].P, (size_t)nblocks, 1.0);
        if (rc) { fp.destroy(); return rc; }
        ffts.push_back(fp); fft_first.push_back(c);
        c = e;
    }
    if (n_analytic) {
        if ((rc = mem.alloc(&xa, 2 * rs * (size_t)(max_batch * M)))) return rc;
        if (AnalyticFft::supports(dtype, M)) {
            ana = new AnalyticFft();
            if ((rc = ana->create(M, max_batch))) return rc;
        } else {
            rc = inv_m.create(1, dtype, (size_t)M, (size_t)max_batch, 1.0 / (double)M);
            if (rc) return rc;
        }
    }
    n_generic = d.n_generic;
    // (SSQ_DEBUG_BLOCK_SPECTRA=rocfft: every class through gather + rocFFT, as in rounds 1-4)
    own4096 = dtype == SSQ_F32 && M > 4096 && !env_equals("SSQ_DEBUG_BLOCK_SPECTRA", "rocfft");
    // (SSQ_DEBUG_BLOCK_SPECTRA=4096: the one-launch kernel for the P = 4096 classes only, as until round 6's second half)
    own_big = own4096 && !env_equals("SSQ_DEBUG_BLOCK_SPECTRA", "4096");
    // (SSQ_DEBUG_BLOCK_PAIRED=0: the Unpaired builds; SSQ_DEBUG_BLOCK_BAND=0: the BandOut builds -- the same bits, for tests)
    paired = !env_is_zero("SSQ_DEBUG_BLOCK_PAIRED");
    band = !env_is_zero("SSQ_DEBUG_BLOCK_BAND");
    {   // the CU count of the device the plan lives on (the multi-class launch asks how full a launch is)
        int dev = 0; hipDeviceProp_t pr;
        bool lds128 = false;                       // (block_spectra_multi_kernel<4>: 128 KB of LDS; gfx950 has 160 KB)
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) {
            ncu = pr.multiProcessorCount;
            lds128 = (size_t)pr.maxSharedMemoryPerMultiProcessor >= 128 * 1024;
        }
        own_big = own_big && lds128;
    }
    return 0;
}

void BlockPlan::destroy() {
    for (auto& f : ffts) f.destroy();
    inv_m.destroy();
    if (ana) { ana->destroy(); delete ana; ana = nullptr; }
    mem.release();
}

int64_t BlockPlan::bytes() const {
    int64_t b = mem.bytes() + (int64_t)inv_m.work_bytes + (ana ? ana->mem.bytes() : 0);
    for (const FftPlan& f : ffts) b += (int64_t)f.work_bytes;
    return b;
}

template <int L>
static int launch_zoom(const BlockArgs& A, const SsqParams& sp, int nsig, bool paired, bool band, hipStream_t stream) {
    if (A.n_items == 0) return 0;
    const dim3 grid((unsigned)A.n_items, (unsigned)nsig);
    return dispatch_zoom_build(A.wx_alone(), A.lean(), paired, band, [&](auto build) {
        hipLaunchKernelGGL((blockzoom_kernel<L, decltype(build)>), grid, dim3(NT), 0, stream, A, sp);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int BlockPlan::run(int sig, int nsig, float* Wx, float* dWx, float* w, unsigned short* kidx,
                   const float* row_scale, double dt, const SsqParams& sp, hipStream_t stream,
                   const int64_t* limit) {
    BlockArgs A;
    A.rows = rows; A.classes = classes; A.pbank = (const float*)pbank; A.pxi = (const float*)pxi;
    A.ctw = (const c32*)ctw;
    A.xb = (const c32*)xb; A.row_scale = row_scale;
    A.Wx = Wx; A.dWx = dWx; A.w = w; A.kidx = kidx;
    A.M = M; A.N = N; A.na = na;
    A.h = (2.0 * 3.141592653589793) / (double)M;
    A.inv_dt = 1.0f / (float)dt;
    A.gamma = sp.gamma; A.sig = sig;
    {   // A transform too small to fill the GPU class by class (C1: five launches of 10-18 us each): one launch.
        // (SSQ_DEBUG_CWT_BLOCKS_MULTI=0/1 forces; default: when no class has more than two workgroups per CU)
        const char* fe = getenv("SSQ_DEBUG_CWT_BLOCKS_MULTI");                 // (read per call: tests switch it)
        const int force = fe ? atoi(fe) : -1;
        int64_t total = 0, biggest = 0; int used = 0;
        for (int s = 0; s < 5; ++s) {
            const int64_t n = limit ? limit[s] : n_items[s];
            total += n; biggest = std::max(biggest, n * nsig); used += n > 0;
        }
        // (... or when the whole call is only a few rounds of workgroups -- three of them share a CU: a single signal
        // at config 2 is 1512 + 1344 workgroups, two rounds per class launched one after the other, 3.7 rounds
        // together: block stage 107 -> 89 us, round 5)
        // (... and the fused form's lean kernels always: at config 2, 16 signals per launch, the two large classes in
        // one launch take 58.5 us per transform against 64.0 one after the other -- one tail instead of two -- round 5)
        const bool multi = force >= 0 ? force != 0
                                      : (used > 1 && (A.lean() || biggest <= 2 * (int64_t)ncu || total * nsig <= 18 * (int64_t)ncu));
        if (multi && total > 0) {
            BlockMultiArgs Mx;
            Mx.A = A; Mx.A.items = nullptr; Mx.A.n_items = total; Mx.A.ftw = nullptr;
            int acc = 0;
            for (int s = 0; s < 5; ++s) {
                Mx.items[s] = (const int4*)items[s]; Mx.ftw[s] = (const c32*)ftw + ftw_off[s];
                Mx.first[s] = acc; acc += (int)(limit ? limit[s] : n_items[s]);
            }
            Mx.first[5] = acc;
            const dim3 grid((unsigned)total, (unsigned)nsig);
            return dispatch_zoom_build(A.wx_alone(), A.lean(), paired, band, [&](auto build) {
                hipLaunchKernelGGL((blockzoom_multi_kernel<decltype(build)>), grid, dim3(NT), 0, stream, Mx, sp);
                SSQ_LAUNCH_CHECK();
                return 0;
            });
        }
    }
    for (int s = 0; s < 5; ++s) {                  // the plan's item lists: L' = 128 << s
        A.items = (const int4*)items[s]; A.n_items = limit ? limit[s] : n_items[s];
        A.ftw = (const c32*)ftw + ftw_off[s];
        const int rc = fft_dispatch<128, 2048>(128 << s, [&](auto len) { return launch_zoom<decltype(len)::value>(A, sp, nsig, paired, band, stream); });
        if (rc) return rc;
    }
    return 0;
}

#include "ssq_block_exact.inl"

}  // namespace ssq
