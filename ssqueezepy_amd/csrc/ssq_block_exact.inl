// ssq_block_exact.inl -- the exact rows of a float32 block plan. Included by ssq_cwt_blocks.hip inside namespace ssq.
// Rows whose impulse response is not compact (pass-band cut by the Nyquist frequency)
// get the reference's full-length transform, as a four-step FFT over M = A x B with
// one intermediate array Z in HBM (the only one on the fast path; ~4 MB per row):
//   pass 1: for every k1 < A, B-point iFFT over k2 of X[k1 + A k2] = psih[k] xh[k]
//           (and of the derivative spectrum), times e^{2 pi i k1 n2 / M} / M. The
//           twiddle is the product of two small per-workgroup LDS tables
//           (n2 = 32 n2_hi + n2_lo), not a gather from the M-entry table per point.
//   pass 2: for every n2 < B, A-point iFFT over k1 of Z[k1][n2] -> y[n2 + B n1],
//           fused with the same unpad / phase / bin-map epilogue as the block kernel.
// Z is stored blocked for pass 2: [n2 / G2][k1][n2 % G2] with G2 the number of n2
// columns a pass-2 workgroup owns, so that a pass-2 workgroup reads one contiguous
// A*G2*8-byte slab and pass 1 (which transposes through LDS) writes G1*G2*8-byte runs.
struct ExactArgs {
    const float* bank; const int64_t* band_off; const int32_t* band_lo;
    const int32_t* rows; const c32* xh; c32* Z; const c32* twM; const c32* ftw;
    const float* row_scale;
    float* Wx; float* dWx; float* w; unsigned short* kidx;
    int64_t M, N, na; int A, B, n1pad, sig, n_rows;   // sig: first signal (blockIdx.z adds)
    int G2;                                           // n2 columns per pass-2 workgroup
    double h; float inv_dt; double gamma;
    bool lean() const { return kidx && !dWx && !w && !row_scale; }     // (as BlockArgs)
};

template <int L>
__global__ __launch_bounds__(NT) void exact_pass1_kernel(ExactArgs E) {
    __shared__ c32 buf[D_POINTS + 64];
    using S = FftShape<L>;
    constexpr int G = S::G, R1 = S::R1, RL = S::RL;
    const int tid = threadIdx.x, r = blockIdx.y, row = E.rows[r];
    const int c0 = blockIdx.x * G;                          // first k1 of this workgroup
    const int lo = E.band_lo[row];
    const int64_t off0 = E.band_off[row];
    const int len = (int)(E.band_off[row + 1] - off0);
    const float* psi = E.bank + off0;
    const c32* xh = E.xh + (int64_t)(E.sig + (int)blockIdx.z) * (E.M / 2 + 1);
    c32 zw[PPT], zd[PPT];
    {
        constexpr int NB = PPT / R1, STR = L / R1;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < R1; ++k) {
                const int kk = (c0 + g) + E.A * (u + k * STR);       // DFT bin
                const int off = kk - lo;
                c32 z = {0.f, 0.f}, dz = {0.f, 0.f};
                if (off >= 0 && off < len) {
                    const float p = psi[off];
                    const c32 X = xh[kk];
                    z = {p * X.x, p * X.y};
                    const float mm = (float)((double)kk * E.h) * E.inv_dt;
                    dz = {-(z.y * mm), z.x * mm};
                }
                zw[it * R1 + k] = z; zd[it * R1 + k] = dz;
            }
        }
    }
    // twiddle tables of this workgroup's G values of k1: e^{2 pi i k1 n2 / M} / M =
    // thi[g][n2 >> 5] * tlo[g][n2 & 31]
    constexpr int NH = (L + 31) / 32;
    __shared__ c32 tlo[G * 32], thi[G * NH];
    {
        const float fM = (float)E.M;                          // power of two: exact
        for (int i = tid; i < G * 32; i += NT)
            tlo[i] = E.twM[(unsigned)(c0 + i / 32) * (unsigned)(i % 32)];
        for (int i = tid; i < G * NH; i += NT) {
            const c32 t = E.twM[(unsigned)(c0 + i / NH) * (unsigned)((i % NH) * 32)];   // < M
            thi[i] = {t.x * fM, t.y * fM};
        }
    }
    constexpr int NBL = PPT / RL, STRL = L / RL;
    const int G2 = E.G2, lg2 = __ffs(G2) - 1;
    constexpr int LG = ilog2(G);
#pragma unroll
    for (int tr = 0; tr < 2; ++tr) {
        c32 (&v)[PPT] = tr ? zd : zw;
        lds_ifft<L>(v, buf, E.ftw, tid);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NBL; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < RL; ++k) {
                const int n2 = u + k * STRL;
                const c32 tw = cmul_v(thi[g * NH + (n2 >> 5)], tlo[g * 32 + (n2 & 31)]);
                buf[g * (L + 1) + n2] = cmul_v(v[it * RL + k], tw);
            }
        }
        __syncthreads();
        c32* Zt = E.Z + (((int64_t)blockIdx.z * E.n_rows + r) * 2 + tr) * E.M;
#pragma unroll
        for (int it = 0; it < PPT; ++it) {
            // consecutive lanes: n2 % G2 fastest, then this workgroup's k1 -> G*G2-element runs
            // (G2 and G are powers of two: shifts, not divisions)
            const int idx = tid + it * NT, n2i = idx & (G2 - 1), g = (idx >> lg2) & (G - 1);
            const int n2t = idx >> (lg2 + LG), n2 = (n2t << lg2) + n2i;
            Zt[((int64_t)n2t * E.A + (c0 + g)) * G2 + n2i] = buf[g * (L + 1) + n2];
        }
    }
}

template <int L, bool LEAN>
__global__ __launch_bounds__(NT) void exact_pass2_kernel(ExactArgs E, SsqParams sp) {
    __shared__ c32 buf[D_POINTS];
    using S = FftShape<L>;
    constexpr int G = S::G, R1 = S::R1;
    const int tid = threadIdx.x, r = blockIdx.y, row = E.rows[r];
    // a workgroup writes G consecutive outputs per n1 (G*8-byte pieces of Wx, G*2 of the bin map):
    // give each XCD (workgroup b -> XCD b % 8) a contiguous range of n2 so the pieces of one
    // line meet in one L2
    const int bx = (gridDim.x & 7) ? (int)blockIdx.x
                                   : (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
    const int c0 = bx * G;                                  // first n2 of this workgroup
    const c32* ZW = E.Z + (((int64_t)blockIdx.z * E.n_rows + r) * 2) * E.M;
    const c32* ZD = ZW + E.M;
    c32 zw[PPT], zd[PPT];
    {
        constexpr int NB = PPT / R1, STR = L / R1;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < R1; ++k) {
                const int64_t q = (int64_t)bx * E.A * G + (u + k * STR) * G + g;   // blocked Z
                zw[it * R1 + k] = ZW[q]; zd[it * R1 + k] = ZD[q];
            }
        }
    }
    lds_ifft<L>(zw, buf, E.ftw, tid);
    lds_ifft<L>(zd, buf, E.ftw, tid);
    const EmitRow er = make_emit_row(E.Wx, E.dWx, E.w, E.kidx, E.row_scale, E.sig + (int)blockIdx.z, (int)blockIdx.z, row, E.na, E.N, E.gamma, sp.flipud);
    const int N = (int)E.N;                                 // (the epilogue of blockzoom_body with another column map)
    constexpr int RL = S::RL, NB = PPT / RL, STR = L / RL;
    unsigned pend = 0;
    auto emit_all = [&](auto grid_tag) {
        constexpr int GRID = decltype(grid_tag)::value;
#pragma unroll
        for (int it = 0; it < NB; ++it) {
            const int idx = tid + it * NT, g = idx % G, u = idx / G;
#pragma unroll
            for (int k = 0; k < RL; ++k) {
                const int n = (c0 + g) + E.B * (u + k * STR);
                const int j = n - E.n1pad;
                if ((unsigned)j >= (unsigned)N) continue;
                if (emit_point<LEAN, GRID>(er, j, zw[it * RL + k], zd[it * RL + k], sp))
                    pend |= 1u << (it * RL + k);
            }
        }
    };
    dispatch_grid<LEAN>(sp.grid, emit_all);
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
                    W = zw[it * RL + k]; D = zd[it * RL + k]; j = (c0 + g) + E.B * (u + k * STR) - E.n1pad;
                }
        }
        if (low) emit_point_exact(er, er.k + j, W, D, sp);
    }
}

// ---- host side
int BlockPlan::setup_exact(const float* bank_dev, const int64_t* band_off_dev, const int32_t* band_lo_dev,
                           const int32_t* gen_rows_dev, const std::vector<int64_t>& h_off,
                           const std::vector<int32_t>& h_lo, const std::vector<int32_t>& h_gen) {
    exact_ok = false;
    if (h_gen.empty()) return 0;
    const int lm = fft_slot(M, 1);                  // (log2 M when M is a power of two)
    if ((1ll << lm) != M || lm < 14 || lm > 22) return 0;
    for (int32_t i : h_gen) {                       // analytic rows only
        int64_t len = h_off[i + 1] - h_off[i];
        if (h_lo[i] + len > M / 2 + 1) return 0;
    }
    exA = 1 << ((lm + 1) / 2); exB = (int)(M / exA);
    e_bank = bank_dev; e_off = band_off_dev; e_lo = band_lo_dev; e_rows = gen_rows_dev;
    n_exact = (int)h_gen.size();
    std::vector<float> tw((size_t)2 * M);
    for (int64_t q = 0; q < M; ++q) {
        double ang = 2.0 * 3.14159265358979323846 * (double)q / (double)M;
        tw[2 * q] = (float)(cos(ang) / (double)M); tw[2 * q + 1] = (float)(sin(ang) / (double)M);
    }
    int rc;
    if ((rc = mem.upload(&twM, tw.data(), 8 * (size_t)M))) return rc;
    if ((rc = mem.alloc(&zbuf, (size_t)group * n_exact * 2 * M * 8))) return rc;
    exact_ok = true;
    return 0;
}

template <int L>
static int launch_exact1(const ExactArgs& E, int n_rows, int nsig, hipStream_t stream) {
    hipLaunchKernelGGL((exact_pass1_kernel<L>), dim3((unsigned)(E.A / FftShape<L>::G), (unsigned)n_rows, (unsigned)nsig),
                       dim3(NT), 0, stream, E);
    SSQ_LAUNCH_CHECK();
    return 0;
}
template <int L>
static int launch_exact2(const ExactArgs& E, const SsqParams& sp, int n_rows, int nsig, hipStream_t stream) {
    const dim3 grid((unsigned)(E.B / FftShape<L>::G), (unsigned)n_rows, (unsigned)nsig);
    return dispatch_bool(E.lean(), [&](auto lean) {
        hipLaunchKernelGGL((exact_pass2_kernel<L, decltype(lean)::value>), grid, dim3(NT), 0, stream, E, sp);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int BlockPlan::run_exact(int sig, int nsig, const void* xh_all, float* Wx, float* dWx, float* w,
                         unsigned short* kidx, const float* row_scale, double dt, const SsqParams& sp,
                         hipStream_t stream) {
    ExactArgs E;
    E.bank = e_bank; E.band_off = e_off; E.band_lo = e_lo; E.rows = e_rows;
    E.xh = (const c32*)xh_all; E.Z = (c32*)zbuf; E.twM = (const c32*)twM; E.row_scale = row_scale;
    E.Wx = Wx; E.dWx = dWx; E.w = w; E.kidx = kidx;
    E.M = M; E.N = N; E.na = na; E.A = exA; E.B = exB; E.n1pad = (int)n1; E.sig = sig; E.n_rows = n_exact;
    E.G2 = D_POINTS / exA;
    E.h = (2.0 * 3.141592653589793) / (double)M; E.inv_dt = 1.0f / (float)dt; E.gamma = sp.gamma;
    // (setup_exact keeps both factors inside 128 .. 2048, the lengths of the plan's twiddle tables)
    const int rc = fft_dispatch<128, 2048>(exB, [&](auto len) {
        E.ftw = (const c32*)ftw + ftw_off[fft_slot(decltype(len)::value, 128)];
        return launch_exact1<decltype(len)::value>(E, n_exact, nsig, stream);
    });
    if (rc) return rc;
    return fft_dispatch<128, 2048>(exA, [&](auto len) {
        E.ftw = (const c32*)ftw + ftw_off[fft_slot(decltype(len)::value, 128)];
        return launch_exact2<decltype(len)::value>(E, sp, n_exact, nsig, stream);
    });
}
