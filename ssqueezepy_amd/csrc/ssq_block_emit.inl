// ssq_block_emit.inl -- per-point pieces of the float32 block rows' fused epilogue (store, phase transform, bin map).
// Included by ssq_cwt_blocks.hip in namespace ssq; the zoom kernels and exact_pass2_kernel (ssq_block_exact.inl) end in them.
// ---- per-point output of the fused epilogues (unpadded Wx [, dWx, w, bin map])
struct EmitRow {
    float2* W; float2* D; float* w; unsigned short* k;
    float rs; bool scale; double gamma; int64_t omax;
    float m2hi, m2lo;          // |Wx|^2 screens of mag_gt (ssq_point_math.inl)
    int fx, fa;                // flipud as (k ^ fx) + fa: (-1, omax + 1) or (0, 0)
};
__device__ __forceinline__ EmitRow make_emit_row(float* Wx, float* dWx, float* w, unsigned short* kidx,
                                                 const float* row_scale, int sig, int ksig, int row,
                                                 int64_t na, int64_t N, double gamma, int flipud) {
    EmitRow e;
    const int64_t base = ((int64_t)sig * na + row) * N;
    e.W = reinterpret_cast<float2*>(Wx) + base;
    e.D = dWx ? reinterpret_cast<float2*>(dWx) + base : nullptr;
    e.w = w ? w + base : nullptr;
    e.k = kidx ? kidx + (int64_t)ksig * na * N + kidx_index(row, 0, na, N) : nullptr;
    e.scale = row_scale != nullptr;
    e.rs = row_scale ? row_scale[row] : 1.f;
    e.gamma = gamma; e.omax = na - 1;
    const float g2 = (float)(gamma * gamma);
    e.m2hi = g2 * 1.000004f; e.m2lo = g2 * 0.999996f;
    e.fx = flipud ? -1 : 0; e.fa = flipud ? (int)na : 0;
    return e;
}
// Stores one point. Returns true when its bin could not be decided by the float32
// screens: the caller then runs `emit_point_exact` for it outside the unrolled loop
// (one copy of the double-precision code per kernel instead of one per point -- the
// unrolled epilogue stays small enough for the instruction cache).
// LEAN: the fused ssq_cwt form (Wx + bin map only) -- the kernels are instantiated
// separately for it so that its epilogue carries no code for the optional outputs, and
// its bin screen is the branch-free one, specialised per grid kind (GRID).
template <bool LEAN, int GRID>
__device__ __forceinline__ bool emit_point(const EmitRow& e, int j, c32 W, c32 D, const SsqParams& sp) {
    float c = W.x, d = W.y, a = D.x, b = D.y;
    if constexpr (LEAN) {                    // lean kernels run without row scaling
        e.W[(unsigned)j] = make_float2(c, d);
        const float m2 = c * c + d * d, num = b * c - a * d;
        const bool above = m2 > e.m2hi, below = m2 < e.m2lo;
        // hardware reciprocal: relative error of w under 3e-7 (see bin_of_point)
        const float w32 = fabsf(num * __builtin_amdgcn_rcpf(m2 * 6.2831855f));
        bool ok;
        const int kb = bin_screen_cwt<GRID>(w32, sp, (int)e.omax, ok);
        const int kf = (kb ^ e.fx) + e.fa;
        e.k[(unsigned)j] = (unsigned short)(above ? kf : 0xFFFF);   // overwritten by the exact path if undecided
        return !(below | (above & ok));
    } else {
        c = c * e.rs; d = d * e.rs; a = a * e.rs; b = b * e.rs;        // rs == 1 (exact) when unscaled
        e.W[j] = make_float2(c, d);
        if (e.D) e.D[j] = make_float2(a, b);
        if (e.w) {
            float wv;
            if (mag_lt(c, d, (float)e.gamma)) wv = INFINITY;
            else wv = (float)fabs(phase_ratio(a, b, c, d));
            e.w[j] = wv;
        }
        if (e.k) {
            const int above = mag_gt_screen(c, d, e.gamma);
            if (above < 0) return true;
            unsigned short kk = 0xFFFFu;
            if (above) {
                const int kb = bin_of_point_screen(a, b, c, d, sp, (int)e.omax);
                if (kb == -2) return true;
                kk = (unsigned short)(sp.flipud ? (int)e.omax - kb : kb);
            }
            e.k[j] = kk;
        }
        return false;
    }
}
// run the epilogue specialised for the grid kind (lean kernels) or generically
template <int V> struct GridTag { static constexpr int value = V; };
template <bool LEAN, typename F>
__device__ __forceinline__ void dispatch_grid(int grid, F&& f) {
    if constexpr (LEAN) {
        if (grid == SSQ_GRID_LOG) f(GridTag<SSQ_GRID_LOG>{});
        else if (grid == SSQ_GRID_LOG_PIECEWISE) f(GridTag<SSQ_GRID_LOG_PIECEWISE>{});
        else f(GridTag<SSQ_GRID_LIN>{});
    } else {
        f(GridTag<-1>{});
    }
}
__device__ __forceinline__ void emit_point_exact(const EmitRow& e, unsigned short* kout, c32 W, c32 D,
                                                 const SsqParams& sp) {
    const float c = W.x * e.rs, d = W.y * e.rs, a = D.x * e.rs, b = D.y * e.rs;
    unsigned short kk = 0xFFFFu;
    if (mag_of(c, d) > e.gamma) {
        const int64_t kb = bin_of_point_exact(a, b, c, d, sp, e.omax);
        kk = (unsigned short)(sp.flipud ? e.omax - kb : kb);
    }
    *kout = kk;
}
