// ssq_block_spectra.inl -- the spectra X_b of a block plan's signal blocks, which the zoom kernels read: gather +
// rocFFT, or one launch of the library's own kernels. Included by ssq_cwt_blocks.hip inside namespace ssq.

// gather the overlapping blocks of the (periodic) padded signals, all classes in one
// launch (blockIdx.y = class)
// T: the element gathered -- a real sample of the padded signal (classes over x, into `blocks`)
// or a complex sample of its analytic signal (classes with analytic = 1, straight into their
// slots of `xb`, transformed in place)
template <typename T, bool ANALYTIC>
__global__ __launch_bounds__(256) void gather_blocks_kernel(const T* __restrict__ xp,
                                                            T* __restrict__ dst,
                                                            const BlockClassDev* __restrict__ classes,
                                                            int64_t M, int64_t n1, int64_t batch) {
    const BlockClassDev k = classes[blockIdx.y];
    const int64_t total = batch * k.nb * k.P;
    const int64_t lead = (k.P == M) ? 0 : n1 - k.m;       // the single-block class starts at 0
    T* out = dst + (ANALYTIC ? k.xb_off : k.blk_off);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = t % k.P, bb = t / k.P, b = bb % k.nb, s = bb / k.nb;
        int64_t src = (lead + b * k.V + p) % M;
        if (src < 0) src += M;
        out[t] = xp[s * M + src];
    }
}

// One-sided spectrum of the analytic signal: X_a[k] = xh[k] for k < M / 2, half of it at the
// Nyquist bin (the bank's halving of that bin, wavelets.py:86-95, moved to the signal -- exact),
// zero above. The inverse transform of it follows in place.
template <typename C>
__global__ __launch_bounds__(256) void analytic_spectrum_kernel(const C* __restrict__ xh, C* __restrict__ xa,
                                                                int64_t M, int64_t batch) {
    const int64_t half = M / 2, total = batch * M;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = t % M, s = t / M;
        C v; v.x = 0; v.y = 0;
        if (k <= half) {
            v = xh[s * (half + 1) + k];
            if (k == half) { v.x *= 0.5f; v.y *= 0.5f; }      // (exact in either precision)
        }
        xa[t] = v;
    }
}

// ---- block spectra of the P = 4096 classes in ONE launch (float32, round 5) ----------------------------------
// Rounds 1-4: gather kernel per kind -> batched rocFFT (real-to-complex for the blocks of x: two kernels; complex for
// the blocks of the analytic signal) per block length: at config 2 -- where every class has P = 4096 -- five launches
// of 6-30 us per launch group (5 us of 327 per transform at 16 signals, 32 of 430 for a single one). Here a workgroup
// takes TWO consecutive real blocks a, b of a signal as one complex sequence a + ib (or one analytic block), gathers
// them from the periodic padded signal, runs the 4096-point LDS transform of ssq_ldsfft.h (radices 16 x 16 x 16;
// twiddles: the class' own e^{2 pi i q / P} table) and writes the spectra the block kernels read:
//   Z' = sum_p z[p] e^{+2 pi i k p / P} = Z[P - k]  (the transform at hand is the inverse one, unnormalised), so
//   X_a[k] = (Z'[P-k] + conj Z'[k]) / 2,   X_b[k] = (Z'[P-k] - conj Z'[k]) / 2i,   k <= P / 2;   analytic: X[k] = Z'[P-k].
struct BlockSpecArgs {
    const float* xp; const c32* xa; c32* xb;
    const c32* xh;                     // the padded signals' half spectra (block_spectra_multi_kernel: a class with P = M)
    const BlockClassDev* classes; const c32* ctw;
    int64_t M, n1;
    int cls[8]; int first[9];          // classes served, first workgroup of each (first[n]: the grid's x size)
    int ncls;
};
__global__ __launch_bounds__(NT) void block_spectra4096_kernel(BlockSpecArgs A) {
    constexpr int P = 4096;
    __shared__ c32 buf[P];
    const int tid = threadIdx.x;
    int b = (int)blockIdx.x, c = 0;
    while (c + 1 < A.ncls && b >= A.first[c + 1]) ++c;
    b -= A.first[c];
    const BlockClassDev k = A.classes[A.cls[c]];
    const int64_t sig = blockIdx.y, M = A.M;
    const int64_t lead = A.n1 - k.m;
    c32 z[PPT];
    const bool ana = k.analytic != 0;
    const int b0 = ana ? b : 2 * b, b1 = b0 + 1;                 // blocks of this workgroup
    const bool two = !ana && b1 < (int)k.nb;
#pragma unroll
    for (int t = 0; t < PPT; ++t) {
        const int p = tid + t * NT;
        int64_t s0 = (lead + (int64_t)b0 * k.V + p) % M; if (s0 < 0) s0 += M;
        if (ana) z[t] = A.xa[sig * M + s0];
        else {
            int64_t s1 = (lead + (int64_t)b1 * k.V + p) % M; if (s1 < 0) s1 += M;
            z[t] = {A.xp[sig * M + s0], two ? A.xp[sig * M + s1] : 0.f};
        }
    }
    lds_ifft<P>(z, buf, A.ctw + k.ctw_off, tid);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PPT; ++t) buf[tid + t * NT] = z[t];    // natural order: Z'[tid + 256 t]
    __syncthreads();
    c32* out0 = A.xb + k.xb_off + (sig * k.nb + b0) * k.xb_stride;
    if (ana) {
#pragma unroll
        for (int t = 0; t < PPT; ++t) { const int f = tid + t * NT; out0[f] = buf[(P - f) & (P - 1)]; }
    } else {
        c32* out1 = out0 + k.xb_stride;
        for (int f = tid; f <= P / 2; f += NT) {
            const c32 Pk = buf[f], Qk = buf[(P - f) & (P - 1)];
            out0[f] = {0.5f * (Qk.x + Pk.x), 0.5f * (Qk.y - Pk.y)};
            if (two) out1[f] = {0.5f * (Qk.y + Pk.y), 0.5f * (Pk.x - Qk.x)};
        }
    }
}

// ---- block spectra of the P = 4096 / 8192 / 16384 classes in ONE launch (float32; small calls, round 6) ---------
// A short signal's plan (config 1: N = 10 000, M = 16 384) has classes of P = 8192 and 16 384 next to the P = 4096
// ones, and their spectra went gather kernel -> rocFFT's two-kernel transforms -> real-to-complex post-processing, six
// launches of 3-7 us in a row on a call of 0.1 ms. Here one launch serves every class. A workgroup has 256 QMAX
// threads (QMAX = the longest block / 4096 = 2 or 4) and runs CW = 4 QMAX columns of 1024 points through lds_ifft at
// once (16 points per thread as everywhere; measured no faster than QMAX columns of 4096 points, whose passes' LDS
// accesses conflict far more -- "r7c" / "r7d" of profiles/r6_ab_history.txt: the banks are not what bounds a launch of a
// few workgroups): a block of P = 1024 C points is its C interleaved sub-sequences y[j C + r]
// (the class' e^{2 pi i q / P} table read at every C-th entry), so a workgroup holds CW / C blocks ("slots": pairs of
// real blocks as one complex sequence, or one analytic block, as above), and the last radix-C step
//   Y'[f + 1024 s] = sum_r e^{2 pi i r f / P} e^{2 pi i r s / C} Z'_r[f]
// goes through LDS (the C terms of an f sit in C different lanes). LDS: 32 QMAX KB (static; gfx950: 160 KB).
// Latency, not throughput, is what this kernel is for: BlockPlan::spectra uses it when the launch is at most a couple
// of workgroups per CU and leaves long batches of P > 4096 blocks to gather + rocFFT.
constexpr int WIDE_L = 1024;
// the columns' transform: radices 16 x 8 x 8; entry z[k] = column g's point u + 64 k (g = tid % CW, u = tid / CW);
// exit z[8 it + k] = its output u' + 128 k, u' = (tid + it NTH) / CW. Its twiddles e^{2 pi i q / 1024} come from an
// 8 KB table in LDS (wide_stage_tw: every C-th entry of the class' table, one coalesced read at the kernel's start,
// beside the signal's loads, instead of two dependent table reads per transform: "r7e" -- worth 14 of 47 us to a kernel
// that ran two transforms in a row in one workgroup, nothing measurable to this one).
template <int CW, int C>
__device__ __forceinline__ void wide_stage_tw(c32* __restrict__ stw, const c32* __restrict__ tw, int tid) {
    for (int i = tid; i < WIDE_L; i += 64 * CW) stw[i] = tw[i * C];
}
template <int CW>
__device__ __forceinline__ void wide_ifft(c32 (&z)[PPT], c32* __restrict__ buf, const c32* __restrict__ stw, int tid) {
    lds_ifft<WIDE_L, false, false, 1, 64 * CW>(z, buf, stw, tid);   // (its first barrier: stw is in place)
}
// the last step's twiddles e^{2 pi i r f / P} of a thread's (slot, f) pairs: asked for at the kernel's start
template <int CW, int C>
__device__ __forceinline__ void wide_load_w(c32 (&w)[PPT / C][C], const c32* __restrict__ tw, int tid) {
#pragma unroll
    for (int i = 0; i < PPT / C; ++i) {
        const int f = (tid + i * 64 * CW) % WIDE_L;
        w[i][0] = {1.f, 0.f};
#pragma unroll
        for (int r = 1; r < C; ++r) w[i][r] = tw[r * f];
    }
}
// wide_natural: the transforms' outputs -> buf[slot P + n] = Y'_slot[n] in natural order, behind a barrier.
// In between, Z'_r[n] sits at [slot][r][(n + 4 r) mod 1024]: the rotation keeps both the writes (a wavefront's lanes
// differ in r first) and the reads (consecutive n) off each other's banks.
template <int CW, int C>
__device__ __forceinline__ void wide_natural(const c32 (&z)[PPT], c32* __restrict__ buf, const c32 (&w)[PPT / C][C], int tid) {
    constexpr int L = WIDE_L, P = L * C, NTH = 64 * CW;
    constexpr int NI = PPT / C;                                  // (slot, f) pairs per thread
    __syncthreads();                                             // (the last pass' reads)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * NTH, g = idx % CW, u = idx / CW, slot = g / C, r = g % C;
#pragma unroll
        for (int k = 0; k < 8; ++k) buf[slot * P + r * L + ((u + k * (L / 8) + 4 * r) & (L - 1))] = z[it * 8 + k];
    }
    __syncthreads();
    c32 y[NI][C];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int e = tid + i * NTH, sl = e / L, f = e % L;
#pragma unroll
        for (int r = 0; r < C; ++r) {
            const c32 v = buf[sl * P + r * L + ((f + 4 * r) & (L - 1))];
            y[i][r] = r ? cmul_v(v, w[i][r]) : v;
        }
        Dft<C>::run(y[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int e = tid + i * NTH, sl = e / L, f = e % L;
#pragma unroll
        for (int s2 = 0; s2 < C; ++s2) buf[sl * P + f + s2 * L] = y[i][s2];
    }
    __syncthreads();
}
template <int CW, int C>
__device__ __forceinline__ void block_spectra_wide(const BlockSpecArgs& A, const BlockClassDev& k, int b, c32* __restrict__ buf,
                                                   c32* __restrict__ stw) {
    constexpr int L = WIDE_L, P = L * C, NTH = 64 * CW, SL = CW / C;
    const int tid = threadIdx.x;
    const int g = tid % CW, u = tid / CW, slot = g / C, r = g % C;
    const int64_t sig = blockIdx.y, M = A.M;
    const bool ana = k.analytic != 0;
    const int nunits = ana ? (int)k.nb : ((int)k.nb + 1) / 2;     // a unit: one analytic block or a pair of real ones
    const c32* __restrict__ tw = A.ctw + k.ctw_off;              // e^{2 pi i q / P}
    const c32* __restrict__ xa = A.xa + sig * M;
    const float* __restrict__ xp = A.xp + sig * M;
    const int64_t lead = A.n1 - k.m;
    const int m32 = (int)M;
    wide_stage_tw<CW, C>(stw, tw, tid);
    c32 w[PPT / C][C];
    wide_load_w<CW, C>(w, tw, tid);
    c32 z[PPT];
    {
        const int unit = b * SL + slot;
        const bool live = unit < nunits;
        const int b0 = ana ? unit : 2 * unit, b1 = b0 + 1;
        const bool two = !ana && b1 < (int)k.nb;
        // first sample of each block in the periodic padded signal, reduced once (P <= M: one wrap at most per point)
        int64_t o0 = (lead + (int64_t)b0 * k.V) % M; if (o0 < 0) o0 += M;
        int64_t o1 = (lead + (int64_t)b1 * k.V) % M; if (o1 < 0) o1 += M;
        const int a0 = (int)o0, a1 = (int)o1;
#pragma unroll
        for (int t = 0; t < PPT; ++t) {
            const int p = (u + t * (L / 16)) * C + r;
            int s0 = a0 + p; if (s0 >= m32) s0 -= m32;
            int s1 = a1 + p; if (s1 >= m32) s1 -= m32;
            c32 v = {0.f, 0.f};
            if (live) {
                if (ana) v = xa[s0];
                else v = {xp[s0], two ? xp[s1] : 0.f};
            }
            z[t] = v;
        }
    }
    wide_ifft<CW>(z, buf, stw, tid);
    wide_natural<CW, C>(z, buf, w, tid);
    for (int sl = 0; sl < SL; ++sl) {
        const int unit = b * SL + sl;
        if (unit >= nunits) break;
        const int b0 = ana ? unit : 2 * unit;
        const bool two = !ana && b0 + 1 < (int)k.nb;
        const c32* __restrict__ Y = buf + sl * P;
        c32* out0 = A.xb + k.xb_off + (sig * k.nb + b0) * k.xb_stride;
        if (ana) {
            for (int f = tid; f < P; f += NTH) out0[f] = Y[(P - f) & (P - 1)];
        } else {
            c32* out1 = out0 + k.xb_stride;
            for (int f = tid; f <= P / 2; f += NTH) {
                const c32 Pk = Y[f], Qk = Y[(P - f) & (P - 1)];
                out0[f] = {0.5f * (Qk.x + Pk.x), 0.5f * (Qk.y - Pk.y)};
                if (two) out1[f] = {0.5f * (Qk.y + Pk.y), 0.5f * (Pk.x - Qk.x)};
            }
        }
    }
}
template <int QMAX>
__global__ __launch_bounds__(NT * QMAX) void block_spectra_multi_kernel(BlockSpecArgs A) {
    __shared__ c32 buf[4096 * QMAX];               // 64 / 128 KB
    __shared__ c32 stw[WIDE_L];
    int b = (int)blockIdx.x, c = 0;
    while (c + 1 < A.ncls && b >= A.first[c + 1]) ++c;
    b -= A.first[c];
    const BlockClassDev k = A.classes[A.cls[c]];
    if (k.P == A.M && k.nb == 1 && !k.analytic && A.xh) {
        // one block = the whole periodic signal from sample o on: its spectrum is the signal's own, already there,
        // turned: X_b[k] = xh[k] e^{2 pi i k o / M} -- no transform (config 1's widest class; such a class has one block,
        // and a 16 384-point transform in one workgroup was the launch's longest chain)
        const int64_t M = A.M, sig = blockIdx.y;
        int64_t o = (A.n1 - k.m) % M; if (o < 0) o += M;
        const c32* __restrict__ tw = A.ctw + k.ctw_off;          // e^{2 pi i q / M}
        const c32* __restrict__ xh = A.xh + sig * (M / 2 + 1);
        c32* __restrict__ out0 = A.xb + k.xb_off + sig * k.nb * k.xb_stride;
        const unsigned mask = (unsigned)M - 1u, ou = (unsigned)o;
        for (int f = (int)threadIdx.x; f <= (int)(M / 2); f += NT * QMAX)
            out0[f] = cmul_v(xh[f], tw[((unsigned)f * ou) & mask]);
        return;
    }
    if (k.P == 4096) block_spectra_wide<4 * QMAX, 4>(A, k, b, buf, stw);
    else if (k.P == 8192) block_spectra_wide<4 * QMAX, 8>(A, k, b, buf, stw);
    else if constexpr (QMAX >= 4) block_spectra_wide<4 * QMAX, 16>(A, k, b, buf, stw);
}

int BlockPlan::spectra(const void* xp, const void* xh, int64_t batch, hipStream_t stream,
                       const unsigned char* need) {
    (void)batch;                                   // planned batch: stale rows are ignored later
    // classes are gathered and transformed in runs of equal block length and kind; with `need`,
    // only the runs that hold a needed class (class indices are contiguous per run). The real
    // classes come first, the analytic ones last: one gather launch per kind. The P = 4096 classes of a
    // float32 plan -- the first ones of each kind -- take block_spectra4096_kernel instead (own4096).
    std::vector<char> run_on(ffts.size(), 1);
    int lo[2] = {nc, nc}, hi[2] = {-1, -1};        // needed class range per kind (rocFFT route)
    bool any_analytic = false;
    BlockSpecArgs S;
    S.ncls = 0; S.first[0] = 0;
    int qmax = 1;                                  // longest block the own kernel serves, in units of 4096
    bool prefix[2] = {true, true};
    for (size_t f = 0; f < ffts.size(); ++f) {
        const int a = fft_first[f], b = f + 1 < ffts.size() ? fft_first[f + 1] : nc;
        bool on = !need;
        for (int c = a; c < b && !on; ++c) on = need[c] != 0;
        const int kind = (int)hcls[a].analytic;
        any_analytic = any_analytic || (on && kind);
        int wanted = 0;                            // (classes of this group the kernel's 8 slots would have to take)
        int64_t group_wgs = 0;
        for (int c = a; c < b; ++c) {
            if (need && !need[c]) continue;
            ++wanted;
            group_wgs += kind ? hcls[c].nb : (hcls[c].nb + 1) / 2;
        }
        // P = 4096: always the library's own kernel; P = 8192 / 16384: the one-launch kernel when the launch is small
        // (a call bound by its launches), gather + rocFFT for long batches of such blocks
        const int64_t Pg = hcls[a].P;
        bool whole = Pg == M && !kind && xh;       // blocks as long as the signal, one per signal: no transform at all
        for (int c = a; c < b && whole; ++c) whole = hcls[c].nb == 1;
        const bool small = own_big && M < ((int64_t)1 << 30) && group_wgs * max_batch <= 2 * (int64_t)ncu &&
                           (whole || ((Pg == 8192 || Pg == 16384) && Pg <= M));
        // (the classes the kernel takes are a prefix of their kind: the gather launch below covers ONE class range per kind,
        // and for the analytic kind it writes into the spectra's own storage)
        if (on && own4096 && prefix[kind] && (Pg == 4096 || small) && S.ncls + wanted <= 8) {     // (a ninth: gather + rocFFT, as for other P)
            for (int c = a; c < b; ++c) {
                if (need && !need[c]) continue;
                S.cls[S.ncls++] = c;
                // (a single block as long as the signal takes no transform -- the kernel turns the signal's own spectrum --
                // and does not ask for the wider workgroup)
                const bool twist = Pg == M && hcls[c].nb == 1 && !kind && xh;
                qmax = std::max(qmax, twist ? 2 : (int)(Pg / 4096));      // (the P = 4096-only kernel knows neither)
            }
            on = false;                            // (not through gather + rocFFT)
        }
        run_on[f] = on;
        if (on) prefix[kind] = false;
        if (on) { lo[kind] = std::min(lo[kind], a); hi[kind] = std::max(hi[kind], b - 1); }
    }
    const size_t rs = dtype == SSQ_F32 ? 4 : 8;
    if (any_analytic) {
        // the analytic signal of every padded signal first
        SSQ_REQUIRE(xh && xa, "analytic block classes need the half spectrum");
        if (ana) {
            int rc = ana->run(xh, xa, max_batch, stream);
            if (rc) return rc;
        } else {
            dim3 ga((unsigned)std::min<int64_t>((max_batch * M + 255) / 256, 4096));
            int rc = dispatch_dtype(dtype, [&](auto t) {
                using C = cx<decltype(t)>;
                hipLaunchKernelGGL(analytic_spectrum_kernel<C>, ga, dim3(256), 0, stream, (const C*)xh, (C*)xa, M, max_batch);
                SSQ_LAUNCH_CHECK();
                return 0;
            });
            if (rc) return rc;
            rc = inv_m.execute(xa, nullptr, stream);
            if (rc) return rc;
        }
    }
    if (S.ncls) {
        S.xp = (const float*)xp; S.xa = (const c32*)xa; S.xb = (c32*)xb; S.xh = (const c32*)xh;
        S.classes = classes; S.ctw = (const c32*)ctw; S.M = M; S.n1 = n1;
        // a workgroup of the wide kernel holds qmax / (P / 4096) units of a class (a unit: a pair of real blocks or one
        // analytic block); the P = 4096-only kernel one
        for (int i = 0; i < S.ncls; ++i) {
            const BlockClassDev& k = hcls[S.cls[i]];
            const int64_t units = k.analytic ? k.nb : (k.nb + 1) / 2;
            const int64_t per = std::max<int64_t>(1, qmax / (k.P / 4096));
            S.first[i + 1] = S.first[i] + (int)((units + per - 1) / per);
        }
        const dim3 sg((unsigned)S.first[S.ncls], (unsigned)max_batch);
        if (qmax == 1)
            hipLaunchKernelGGL(block_spectra4096_kernel, sg, dim3(NT), 0, stream, S);
        else if (qmax == 2)
            hipLaunchKernelGGL(block_spectra_multi_kernel<2>, sg, dim3(NT * 2), 0, stream, S);
        else
            hipLaunchKernelGGL(block_spectra_multi_kernel<4>, sg, dim3(NT * 4), 0, stream, S);
        SSQ_LAUNCH_CHECK();
    }
    for (int kind = 0; kind < 2; ++kind) {
        if (hi[kind] < lo[kind]) continue;
        int64_t most = 0;
        for (int c = lo[kind]; c <= hi[kind]; ++c) most = std::max<int64_t>(most, max_batch * hcls[c].nb * hcls[c].P);
        dim3 grid((unsigned)std::min<int64_t>((most + 255) / 256, 2048), (unsigned)(hi[kind] - lo[kind] + 1));
        const int rc = dispatch_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            using C = cx<T>;
            if (kind == 0)
                hipLaunchKernelGGL((gather_blocks_kernel<T, false>), grid, dim3(256), 0, stream, (const T*)xp,
                                   (T*)blocks, classes + lo[0], M, n1, max_batch);
            else
                hipLaunchKernelGGL((gather_blocks_kernel<C, true>), grid, dim3(256), 0, stream, (const C*)xa,
                                   (C*)xb, classes + lo[1], M, n1, max_batch);
            SSQ_LAUNCH_CHECK();
            return 0;
        });
        if (rc) return rc;
    }
    for (size_t f = 0; f < ffts.size(); ++f) {
        if (!run_on[f]) continue;
        const BlockClassDev& k = hcls[fft_first[f]];
        int rc = k.analytic ? ffts[f].execute((char*)xb + (size_t)k.xb_off * 2 * rs, nullptr, stream)
                            : ffts[f].execute((char*)blocks + (size_t)k.blk_off * rs,
                                              (char*)xb + (size_t)k.xb_off * 2 * rs, stream);
        if (rc) return rc;
    }
    return 0;
}
