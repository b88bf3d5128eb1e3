// ssq_conceft.inl -- ssq_conceft, ssq_conceft_cwt: multitaper synchrosqueezing (ConceFT; Daubechies, Wang, Wu 2016) in
// one kernel, in its STFT and its CWT form.
// Included by ssq_kernels.hip inside `namespace ssq`, after the accumulate kernels whose ordered row-lane combine
// (FoldLower) it shares. include/ssq_hip.h states what is computed; DESIGN.md section 4.5.5 the sizing.
//
// A workgroup owns a tile of TC adjacent columns of one signal, a wavefront WC = 4 of them x 16 row-lanes (lane =
// 16 * column + row-lane) -- the float64 layout of accumulate_tile16_kernel. Its wavefronts never synchronise with each
// other: each has its own slab of the LDS tile (rows x 4 complex128 cells, skewed like the tile kernel's), and
// keeps the running sums of the cells k = row-lane + 16 s of its own columns in registers (NC of them per lane).
// Per projection q: the point's J pairs (V_j, dV_j) are loaded (after the first projection they come from the
// caches: a tile's planes are J * rows * TC * 32 bytes at most), mixed in float64 with r[q][.] -- which sits in scalar
// registers, read through the constant address space --, thresholded, mapped to a bin by the exact map and added to
// the tile in ascending row order; then every lane folds its cells into its sums and clears them.
// HBM traffic: the 2J planes once, Cx once; nothing of size (Q, rows, n) exists anywhere.
// CWT = false is ssq_conceft: a row's value is Sfs[i] (the planes' real dtype), w = |Sfs[i] - phase_ratio| and a term is
// Vq. CWT = true is ssq_conceft_cwt: a row's value is the weight cst[i] (float64), w = |phase_ratio| and a term is
// Vq * cst[i]; on the log grids the bin map takes log2(w), inside the branch that a point below gamma skips.
struct ConceftPlanes { const void* v[8]; const void* dv[8]; };

// rows a tile of TC columns supports: TC * 16 bytes per row in 160 KiB of LDS, 16 NC cells per column in registers
constexpr int64_t CONCEFT_MAX_ROWS = 1280;

template <typename T, int TC, int NC, bool CPLX, bool CWT>
__global__ __launch_bounds__(64 * (TC / 4)) void conceft_kernel(
    ConceftPlanes P, const std::conditional_t<CWT, double, T>* __restrict__ Sfs, const double* __restrict__ proj,
    T* __restrict__ Cx, SsqParams sp, int J, int Q, int rows, int n, unsigned tiles) {
    constexpr int RL = 16, WC = 4;
    using TM = Term<double, false>;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int cl = lane / RL, rl = lane % RL;
    const unsigned b = blockIdx.x / tiles, tile_id = blockIdx.x - b * tiles;
    if ((int64_t)tile_id * TC + wave * WC >= n) return;        // (wave-uniform: the wavefront has no column)
    const int j = (int)tile_id * TC + wave * WC + cl;
    const bool col_ok = j < n;
    const int jc = col_ok ? j : n - 1;
    const int64_t omax = rows - 1;
    const size_t boff = (size_t)b * (size_t)rows * (size_t)n;   // (the host guarantees batch rows n < 2^32)
    double* slab = reinterpret_cast<double*>(lds_raw) + (size_t)wave * rows * WC * 2;
    const auto* r = SSQ_CONST_PTR(double, proj);

    for (int t = lane; t < rows * WC * 2; t += 64) slab[t] = 0.0;
    double acc[NC][CPLX ? 2 : 1];
#pragma unroll
    for (int s = 0; s < NC; ++s) { acc[s][0] = 0.0; if constexpr (CPLX) acc[s][1] = 0.0; }
    __builtin_amdgcn_wave_barrier();

    for (int q = 0; q < Q; ++q) {
        const auto* rq = r + 2 * (size_t)q * J;
        for (int i0 = 0; i0 < rows; i0 += RL) {
            const int i = i0 + rl;
            const int ic = i < rows ? i : rows - 1;
            // loads are unconditional (row and column clamped, the point discarded at its use) and all 2J of a
            // point are requested before the first is used
            const size_t off = boff + (size_t)((unsigned)ic * (unsigned)n + (unsigned)jc);
            T zr[8], zi[8], er[8], ei[8];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t < J) {
                    const T* z = (const T*)P.v[t] + 2 * off;
                    const T* e = (const T*)P.dv[t] + 2 * off;
                    zr[t] = z[0]; zi[t] = z[1]; er[t] = e[0]; ei[t] = e[1];
                }
            const double sf = (double)Sfs[ic];
            double vr = 0.0, vi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (t < J) {
                    const double ar = rq[2 * t], ai = rq[2 * t + 1];
                    vr = vr + (ar * (double)zr[t] - ai * (double)zi[t]);
                    vi = vi + (ar * (double)zi[t] + ai * (double)zr[t]);
                    dr = dr + (ar * (double)er[t] - ai * (double)ei[t]);
                    di = di + (ar * (double)ei[t] + ai * (double)er[t]);
                }
            int k = -1;
            if (col_ok && i < rows && !(hypot(vr, vi) < sp.gamma)) {
                if constexpr (CWT) k = (int)bin_from_w(fabs(phase_ratio(dr, di, vr, vi)), sp, omax);
                else k = (int)bin_from_w(fabs(sf - phase_ratio(dr, di, vr, vi)), sp, omax);
                if (sp.flipud) k = (int)omax - k;
            }
            // the 16 rows of the step, combined in registers in ascending row order: one LDS read and one LDS write
            // per cell and step (accumulate_tile16_kernel)
            double tr = 0.0, ti = 0.0, ore = 0.0, oim = 0.0;
            double* cell = slab;
            if (k >= 0) {
                if constexpr (CWT) { tr = vr * sf; ti = vi * sf; }
                else { tr = vr; ti = vi; }
                cell = slab + 2 * (k * WC + ((cl + k) & (WC - 1)));
                ore = cell[0]; oim = cell[1];
            }
            unsigned long long higher = 0;
            const int key = k + 1;
            FoldLower<RL - 1, false, TM, double, double>::run(key, __builtin_amdgcn_ballot_w64(key != 0), tr, ti, ore, oim,
                                                              higher);
            ore = ore + tr; oim = oim + ti;
            if (k >= 0 && !((higher >> lane) & 1ull)) { cell[0] = ore; cell[1] = oim; }
            __builtin_amdgcn_wave_barrier();
        }
        // fold T_q into the running sums and clear it. An empty cell is skipped: it would add +0.
#pragma unroll
        for (int s = 0; s < NC; ++s) {
            const int k = rl + RL * s;
            if (k < rows) {
                double* cell = slab + 2 * (k * WC + ((cl + k) & (WC - 1)));
                const double re = cell[0], im = cell[1];
                if (re != 0.0 || im != 0.0) {
                    if constexpr (CPLX) { acc[s][0] = acc[s][0] + re; acc[s][1] = acc[s][1] + im; }
                    else acc[s][0] = acc[s][0] + hypot(re, im);
                    cell[0] = 0.0; cell[1] = 0.0;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (!col_ok) return;
    const double qd = (double)Q;
#pragma unroll
    for (int s = 0; s < NC; ++s) {
        const int k = rl + RL * s;
        if (k < rows) {
            const size_t o = boff + (size_t)((unsigned)k * (unsigned)n + (unsigned)j);
            if constexpr (CPLX) { Cx[2 * o] = (T)(acc[s][0] / qd); Cx[2 * o + 1] = (T)(acc[s][1] / qd); }
            else Cx[o] = (T)(acc[s][0] / qd);
        }
    }
}

// r[q][j] on the current device, (Q, J, 2) float64: uploaded once per (device, contents) and kept, like the row
// tables of ssq_cwt2_phase -- a call that finds its table enqueues the kernel and nothing else. The eight most
// recent stay; an older one is freed with hipFree, which waits for the kernels that may still read it.
struct ConceftTable { int dev; std::vector<double> proj; double* d; };
static std::mutex g_conceft_mutex;
static std::vector<ConceftTable> g_conceft_tables;

static int conceft_proj_table(const double* proj, size_t count, const double** out) {
    int dev = 0;
    SSQ_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_conceft_mutex);
    for (const ConceftTable& t : g_conceft_tables)
        if (t.dev == dev && t.proj.size() == count && memcmp(t.proj.data(), proj, count * sizeof(double)) == 0) {
            *out = t.d;
            return 0;
        }
    if (g_conceft_tables.size() >= 8) {
        (void)hipFree(g_conceft_tables.front().d);
        g_conceft_tables.erase(g_conceft_tables.begin());
    }
    double* d = nullptr;
    SSQ_CHECK_HIP(hipMalloc((void**)&d, count * sizeof(double)));
    hipError_t e = hipMemcpy(d, proj, count * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); SSQ_CHECK_HIP(e); }
    g_conceft_tables.push_back(ConceftTable{dev, std::vector<double>(proj, proj + count), d});
    *out = d;
    return 0;
}

template <typename T, bool CPLX, bool CWT>
static int launch_conceft(const ConceftPlanes& P, const void* Sfs, const double* proj, void* Cx, const SsqParams& sp,
                          int64_t batch, int64_t J, int64_t Q, int64_t rows, int64_t n, hipStream_t stream) {
    using R = std::conditional_t<CWT, double, T>;             // the row vector's element: Sfs, or the float64 weights
    // the widest tile whose rows fit the LDS and whose cells fit the lanes' registers
#define SSQ_CONCEFT(TC, NC)                                                                                       \
    {                                                                                                             \
        const size_t lds = (size_t)rows * TC * 16;                                                                \
        const unsigned tiles = (unsigned)((n + TC - 1) / TC);                                                     \
        auto kern = conceft_kernel<T, TC, NC, CPLX, CWT>;                                                         \
        SSQ_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                                    \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                 \
        hipLaunchKernelGGL(kern, dim3(tiles * (unsigned)batch), dim3(64 * (TC / 4)), lds, stream, P,              \
                           (const R*)Sfs, proj, (T*)Cx, sp, (int)J, (int)Q, (int)rows, (int)n, tiles);            \
    }
    if (rows <= 16 * 17) SSQ_CONCEFT(16, 17)
    else if (rows <= 16 * 40) SSQ_CONCEFT(16, 40)
    else SSQ_CONCEFT(8, 80)
#undef SSQ_CONCEFT
    SSQ_LAUNCH_CHECK();
    return 0;
}
