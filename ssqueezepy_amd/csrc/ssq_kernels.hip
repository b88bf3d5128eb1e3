// ssq_kernels.hip -- reassignment / phase / framing / padding kernels for gfx950 and
// the runtime half of the C ABI (include/ssq_hip.h).
//
// Compiled with -ffp-contract=off: the per-point arithmetic here is specified
// operation by operation (see oracle/ssq_oracle.c, "numba typing") so that bin
// indices are reproducible bit-for-bit against the CPU path; no fused multiply-adds
// may be introduced behind our back.
//
// Kernel inventory (all HBM-bound streaming kernels; no MFMA -- there is no dense
// contraction on this path):
//   accumulate_tile_kernel   fused phase transform + bin map + accumulate. One
//       wavefront (64 lanes) owns a tile of TC time columns x all `na` frequency
//       bins of Tx, held in LDS (<=160 KiB/CU on gfx950); it streams rows of
//       Wx/dWx through registers with several loads in flight per lane, applies
//       updates in ascending row order (the reference's summation order) and writes
//       the tile out once. HBM traffic = read Wx + dWx (or w / bin map) once, write
//       Tx once -- no read-modify-write, no atomics, deterministic.
//   accumulate_global_kernel fallback for `na` too large for an LDS tile.
//   multi_squeeze_kernel     (ssq_multi_squeeze.inl) the ordered accumulate from `w` iterated on itself: a second LDS
//       slab per wavefront holds its columns of `w`, the iteration is a loop of LDS gathers. Templated on how a
//       frequency becomes a row position: rows at f0 + i df (ssq_multi_squeeze) or at a monotone table kept in LDS and
//       searched per pass (ssq_multi_squeeze_cwt).
//   phase_kernel             w = |Im(dWx/Wx)|/2pi (CWT) or |Sfs - ...| (STFT).
//   stft2_phase_kernel       second-order w of the STFT from five transform planes, float64 in registers.
//   cwt2_phase_kernel        second-order w of the CWT from five transform planes and the rows' scales, likewise.
//       (They share Phase2Vec and launch_phase2; why not more: DESIGN.md section 4.5.3.)
//   replace_under_abs_kernel, buffer_kernel, pad_kernel.
// See also: conceft_kernel (ssq_conceft.hip) and time_reassign_kernel (ssq_time_reassign.hip), which share the ordered
// row-lane combine of accumulate_tile16_kernel through ssq_reassign_dev.h.
#include "ssq_common.h"
#include "ssq_reassign_dev.h"
#include <cfloat>
#include <cstdlib>
#include <string>

namespace ssq {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

#include "ssq_point_math.inl"

// out += z * cst   in the CPU path's arithmetic: Term::fold(o, Term::make(z, w)), kept written out for
// accumulate_tile_kernel -- through Term the float64-weight build converts the cell after the product instead of before
// it and the kernel's instructions come out in another order (profiles/reassign_fold_isa.txt)
template <typename T, bool CST64>
__device__ __forceinline__ void weighted_add(T& o_re, T& o_im, T c, T d, const void* cst, int64_t i) {
    if constexpr (CST64 && sizeof(T) == 4) {
        double w = ((const double*)cst)[i];
        o_re = (T)((double)o_re + (double)c * w);
        o_im = (T)((double)o_im + (double)d * w);
    } else {
        T w = ((const T*)cst)[i];
        o_re = o_re + c * w;
        o_im = o_im + d * w;
    }
}

// Per-point side input of the accumulate kernels, loaded up front so that the loads
// of several rows are in flight together.
template <typename T, int BINSRC> struct SideVal;
template <typename T> struct SideVal<T, BIN_FROM_DWX> {
    static constexpr size_t stride = 2 * sizeof(T);
    T a, b;
    __device__ __forceinline__ void load(const void* src, int64_t q, int64_t, int64_t, int64_t) {
        const T* dz = (const T*)src + 2 * q; a = dz[0]; b = dz[1];
    }
};
template <typename T> struct SideVal<T, BIN_FROM_W> {
    static constexpr size_t stride = sizeof(T);
    T w;
    __device__ __forceinline__ void load(const void* src, int64_t q, int64_t, int64_t, int64_t) { w = ((const T*)src)[q]; }
};
template <typename T> struct SideVal<T, BIN_FROM_KIDX> {
    static constexpr size_t stride = 2;
    unsigned short k;
    __device__ __forceinline__ void load(const void* src, int64_t q, int64_t, int64_t, int64_t) {
        k = ((const unsigned short*)src)[q];
    }
};

// One point of the fused kernel: returns bin (or -1) for row i
template <typename T, int BINSRC, bool STFT>
__device__ __forceinline__ int64_t point_bin(T c, T d, const SideVal<T, BINSRC>& sv, int64_t i,
                                             const T* Sfs, const SsqParams& sp, int64_t omax) {
    int64_t k;
    if constexpr (BINSRC == BIN_FROM_DWX) {
        if (!mag_gt(c, d, sp.gamma)) return -1;
        T sf = T(0);
        if constexpr (STFT) sf = Sfs[i];
        k = bin_of_point(sv.a, sv.b, c, d, STFT, sf, sp, omax);
    } else if constexpr (BINSRC == BIN_FROM_W) {
        if (isinf(sv.w)) return -1;
        k = bin_from_stored_w(sv.w, sp, omax);
    } else {
        if (sv.k == 0xFFFFu) return -1;
        return (int64_t)sv.k;             // already flipped by the producer
    }
    return sp.flipud ? omax - k : k;
}

// ------------------------------------------------- accumulate, LDS-tile form
// block = 64 threads = RL row-lanes x TC columns; tile[k][c] complex<T> in LDS.
template <typename T, int BINSRC, bool STFT, bool CST64, int TC>
__global__ __launch_bounds__(64) void accumulate_tile_kernel(
    const T* __restrict__ Wx, const void* __restrict__ src, const T* __restrict__ Sfs,
    T* __restrict__ Tx, const void* __restrict__ cst, SsqParams sp, int64_t na, int64_t n,
    int32_t* __restrict__ kmap) {
    constexpr int RL = 64 / TC;
    constexpr int U = 4;                       // row batches in flight per lane
    extern __shared__ __align__(16) unsigned char lds_raw[];
    T* tile = reinterpret_cast<T*>(lds_raw);   // [na][TC][2]

    const int lane = threadIdx.x;
    const int c = lane % TC, rl = lane / TC;
    const int64_t j = (int64_t)blockIdx.x * TC + c;
    const int64_t b = blockIdx.y;
    const bool col_ok = j < n;
    const int64_t omax = na - 1;
    const int64_t base = b * na * n;

    for (int64_t t = lane; t < na * TC; t += 64) {
        tile[2 * t] = T(0);
        tile[2 * t + 1] = T(0);
    }
    __builtin_amdgcn_wave_barrier();

    for (int64_t i0 = 0; i0 < na; i0 += RL * U) {
        T zc[U], zd[U];
        SideVal<T, BINSRC> sv[U];
        int64_t kk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t i = i0 + u * RL + rl;
            bool ok = col_ok && i < na;
            zc[u] = T(0); zd[u] = T(0); kk[u] = -1;
            if (ok) {
                int64_t q = base + i * n + j;
                zc[u] = Wx[2 * q];
                zd[u] = Wx[2 * q + 1];
                sv[u].load(src, q, i, j, na);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int64_t i = i0 + u * RL + rl;
            bool ok = col_ok && i < na;
            if (ok) {
                kk[u] = point_bin<T, BINSRC, STFT>(zc[u], zd[u], sv[u], i, Sfs, sp, omax);
                if (kmap) kmap[base + i * n + j] = (int32_t)kk[u];
            }
        }
        // apply in ascending row order: batch u, then row-lane r
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int r = 0; r < RL; ++r) {
                if (rl == r && kk[u] >= 0) {
                    T* o = tile + 2 * (kk[u] * TC + c);
                    T ore = o[0], oim = o[1];
                    weighted_add<T, CST64>(ore, oim, zc[u], zd[u], cst, i0 + u * RL + r);
                    o[0] = ore; o[1] = oim;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (col_ok) {
        for (int64_t k = rl; k < na; k += RL) {
            int64_t q = base + k * n + j;
            Tx[2 * q] = tile[2 * (k * TC + c)];
            Tx[2 * q + 1] = tile[2 * (k * TC + c) + 1];
        }
    }
}

// ------------------------------------- accumulate, LDS-tile form, fast variant
// Same contract as accumulate_tile_kernel, organised for latency hiding. The chain
// "load -> bin -> LDS read -> fold -> LDS write" of one column is serial by
// definition (ascending-row summation order), so the kernel (a) makes the chain short
// and (b) keeps many independent chains per SIMD:
//   * a wavefront owns WC adjacent columns x RL row-lanes (RL = 8, WC = 8 for float32;
//     RL = 16, WC = 4 for float64; lane = RL*col + rl); the RL rows of a step are combined
//     in registers: every lane reads its target cell once, folds in -- in ascending row
//     order, the reference's summation order, bit for bit -- the terms of the lower
//     row-lanes of its column that hit the same cell (DPP row_shr moves), and only the
//     highest lane of a cell writes it back: one LDS read + one LDS write per RL rows;
//   * a workgroup is 16/WC such wavefronts (16 columns, 128-byte row segments between
//     them in float32); its Tx tile (na x 16 cells) lives in LDS, 4 workgroups per CU, and
//     the wavefronts never synchronise with each other;
//   * a few row batches are kept in flight in registers per lane (rolling prefetch of
//     depth U; loads unconditional so that the compiler can count them);
//   * cells are stored skewed (cell (k, c) at WC*k + ((c + k) & (WC-1)) of the wave's
//     slab) to spread the columns of a wave over LDS banks.
// (dpp_mov, Term and FoldLower: ssq_reassign_dev.h)
//
// RL = row-lanes per column (16 or 8): a wavefront covers WC = 64/RL columns and the
// 16-column tile takes 16/WC wavefronts. With RL = 8 two columns share a 16-lane DPP
// row; their keys are made distinct so that a shift across the boundary never matches.
// Fold work per column falls with RL (RL-1 distances per RL rows) and so does the
// number of resident wavefronts (LDS per wavefront grows with WC).
template <typename T, int BINSRC, bool STFT, bool CST64, int U, int WPS, int RL, int TC = 16>
__global__ __launch_bounds__(64 * (TC / (64 / RL)), WPS) void accumulate_tile16_kernel(
    const T* __restrict__ Wx, const void* __restrict__ src, const T* __restrict__ Sfs,
    T* __restrict__ Tx, const void* __restrict__ cst, SsqParams sp, int64_t na64, int64_t n64,
    int32_t* __restrict__ kmap) {
    constexpr int WC = 64 / RL;                    // columns per wavefront
    constexpr int NTH = 64 * (TC / WC);            // threads per workgroup
    using TM = Term<T, CST64>;
    using term_t = typename TM::type;
    using w_t = typename TM::wtype;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int na = (int)na64, n = (int)n64;        // host guarantees na * n < 2^31
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* tile = reinterpret_cast<T*>(lds_raw);       // [4 waves][na][4][2], cells skewed
    T* slab = tile + (size_t)wave * na * WC * 2;
    const int cl = lane / RL, rl = lane % RL;
    const int colkey = (RL < 16) ? ((cl & (16 / RL - 1)) << 20) : 0;   // column tag inside a DPP row

    // XCD-aware tile order (workgroup b runs on XCD b % 8: used for speed only):
    // consecutive 16-column tiles are issued to the same XCD back to back
    const int per = gridDim.x >> 3;                // grid.x is a multiple of 8
    const int tile_id = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile_id * TC >= n) return;
    const int j = tile_id * TC + wave * WC + cl;
    const bool col_ok = j < n;
    const int64_t omax = na - 1;
    const size_t boff = (size_t)blockIdx.y * (size_t)na * (size_t)n;
    const T* Wb = Wx + 2 * boff;
    T* Tb = Tx + 2 * boff;
    int32_t* kb = kmap ? kmap + boff : nullptr;
    const char* sb = (const char*)src + boff * SideVal<T, BINSRC>::stride;

    for (int t = lane; t < na * WC * 2; t += 64) slab[t] = T(0);
    __builtin_amdgcn_wave_barrier();

    // rolling prefetch: slot u holds rows i0 + 16*u + rl; after a slot is consumed the
    // row 16*U further down is requested into it, so 16*U rows per column are in flight
    T zc[U], zd[U];
    w_t wt[U];
    SideVal<T, BINSRC> sv[U];
    const bool uni = sp.cst_uniform != 0;          // scalar weight: one load per kernel
    const w_t w0 = ((const w_t*)cst)[0];
    // Loads are unconditional (row and column clamped into the array, the point is
    // discarded at its use when it lies outside): with a branch around them the compiler
    // loses count of the loads in flight and drains them all (s_waitcnt vmcnt(0)) before
    // every use, which turns the rolling prefetch into one batch at a time.
    const int jc = col_ok ? j : n - 1;
    auto request = [&](int u, int i) {
        const int ic = i < na ? i : na - 1;
        const unsigned q = (unsigned)ic * (unsigned)n + (unsigned)jc;
        zc[u] = Wb[2 * (size_t)q];
        zd[u] = Wb[2 * (size_t)q + 1];
        sv[u].load(sb, q, ic, jc, na);
        if (!uni) wt[u] = ((const w_t*)cst)[ic];
    };
#pragma unroll
    for (int u = 0; u < U; ++u) request(u, u * RL + rl);

    for (int i0 = 0; i0 < na; i0 += RL * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * RL + rl;
            int k = -1;
            if (col_ok && i < na) {
                k = (int)point_bin<T, BINSRC, STFT>(zc[u], zd[u], sv[u], i, Sfs, sp, omax);
                if (kb) kb[(unsigned)i * (unsigned)n + (unsigned)j] = k;
            }
            term_t tr = term_t(0), ti = term_t(0);
            T ore = T(0), oim = T(0);
            T* cell = slab;
            if (k >= 0) {
                const w_t wsel = uni ? w0 : wt[u];
                tr = TM::make(zc[u], wsel);
                ti = TM::make(zd[u], wsel);
                cell = slab + 2 * (k * WC + ((cl + k) & (WC - 1)));
                ore = cell[0]; oim = cell[1];
            }
            request(u, i + RL * U);                 // refill the slot
            unsigned long long higher = 0;
            const int key = k >= 0 ? (k | colkey) + 1 : 0;
            FoldLower<RL - 1, (RL < 16), TM, T, term_t>::run(key, __builtin_amdgcn_ballot_w64(key != 0), tr, ti,
                                                             ore, oim, higher);
            ore = TM::fold(ore, tr); oim = TM::fold(oim, ti);
            const bool last = !((higher >> lane) & 1ull);
            if (k >= 0 && last) { cell[0] = ore; cell[1] = oim; }
            __builtin_amdgcn_wave_barrier();
        }
    }
    // write-out by the whole workgroup: every row of the tile leaves as one 16-column
    // segment (a full 128-byte line in float32), 16 rows per pass
    __syncthreads();
    {
        const int cc = threadIdx.x % TC, rr = threadIdx.x / TC;
        const int jj = tile_id * TC + cc;
        const T* ws = tile + (size_t)(cc / WC) * na * WC * 2;        // owning wave's slab
        const int c4 = cc % WC;
        if (jj < n) {
#pragma unroll 4
            for (int k = rr; k < na; k += NTH / TC) {
                const T* cell = ws + 2 * (k * WC + ((c4 + k) & (WC - 1)));
                size_t q = (size_t)((unsigned)k * (unsigned)n + (unsigned)jj);
                Tb[2 * q] = cell[0];
                Tb[2 * q + 1] = cell[1];
            }
        }
    }
}

// --------------------------------- accumulate from a bin map, float64 tile, unordered
// The bins are known (2-byte map written by the producer), so a point costs two LDS float64
// adds (ds_add_f64, no return value) into a tile of `na` x COLS float64 cells held as a real and
// an imaginary plane: no ordering between rows, hence no combining across lanes and no ticket.
// Each cell is the float64 sum of its terms in whatever order the hardware served them, rounded
// to the data type once at the write-out -- for float32 data that is within 1e-6 of the cell's
// ordered float32 sum (float64 rounding, 1e-16 per add, is far below float32's), for float64
// data within n_terms * 2^-53. SSQ_TILE_ORDER=ordered keeps the bit-exact kernels above.
// A wavefront instruction covers 64 / COLS consecutive rows x COLS columns; loads are
// unconditional (clamped) and refilled as consumed, NW wavefronts share a tile.
bool reassign_ordered() {
    const char* e = getenv("SSQ_TILE_ORDER");       // (read at every launch: tests switch it)
    return e && !strcmp(e, "ordered");
}

template <typename T, bool CST64, int COLS, int NW, int U>
__global__ __launch_bounds__(64 * NW) void accumulate_f64_kernel(
    const T* __restrict__ Wx, const unsigned short* __restrict__ kidx, T* __restrict__ Tx,
    const void* __restrict__ cst, int cst_uniform, int na, int n) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* plane = reinterpret_cast<double*>(lds_raw);
    using TM = Term<T, CST64>;
    using w_t = typename TM::wtype;
    constexpr int RPI = 64 / COLS;                 // rows per wavefront instruction
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane % COLS, h = lane / COLS;
    const int per = gridDim.x >> 3;                // grid.x is a multiple of 8: tiles of one XCD adjoin
    const int tile_id = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile_id * COLS >= n) return;
    const int j = tile_id * COLS + c;
    const bool col_ok = j < n;
    const int jc = col_ok ? j : n - 1;
    const size_t boff = (size_t)blockIdx.y * (size_t)na * (size_t)n;
    const T* Wb = Wx + 2 * boff;
    const unsigned short* kb = kidx + boff;
    T* Tb = Tx + 2 * boff;
    const int cells = na * COLS;
    const unsigned im_off = (unsigned)cells * 8u;  // byte offset of the imaginary plane

    for (int t = tid; t < 2 * cells; t += 64 * NW) plane[t] = 0.0;
    __syncthreads();

    T zc[U], zd[U];
    w_t wt[U];
    unsigned short kk[U];
    const bool uni = cst_uniform != 0;
    auto request = [&](int u, int i) {
        const int ic = i < na ? i : na - 1;
        const unsigned q = (unsigned)ic * (unsigned)n + (unsigned)jc;
        if constexpr (sizeof(T) == 4) {
            const float2 z = reinterpret_cast<const float2*>(Wb)[q];
            zc[u] = z.x; zd[u] = z.y;
        } else {
            // (float64: read once, written once -- nontemporal, config 5 -1.5 ... -2 %, "r6y22")
            typedef double ssq_d2v __attribute__((ext_vector_type(2)));
            const ssq_d2v z = __builtin_nontemporal_load(reinterpret_cast<const ssq_d2v*>(Wb) + q);
            zc[u] = z.x; zd[u] = z.y;
        }
        kk[u] = kb[q];
        wt[u] = ((const w_t*)cst)[uni ? 0 : ic];   // (unconditional: a branch around a load costs a full drain)
    };
    const int step = NW * RPI;                     // rows between two groups of one wavefront
#pragma unroll
    for (int u = 0; u < U; ++u) request(u, (wv + u * NW) * RPI + h);
    for (int i0 = wv * RPI; i0 < na; i0 += U * step) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * step + h;
            const unsigned k = kk[u];
            const w_t wsel = wt[u];
            // the product in the CPU path's arithmetic (float32 data x float32 weight is a float32
            // product; a float64 weight vector makes it a float64 one), the sum in float64
            const double tr = (double)TM::make(zc[u], wsel), ti = (double)TM::make(zd[u], wsel);
            const bool live = col_ok && i < na && k != 0xFFFFu;
            if (live) {
                const unsigned off = (k * (unsigned)COLS + (unsigned)c) * 8u;
                SSQ_LDS_ADD_F64(lds_raw, off, tr);
                SSQ_LDS_ADD_F64(lds_raw, off + im_off, ti);
            }
            request(u, i + U * step);              // refill the slot
        }
    }
    __syncthreads();
    if (col_ok) {
        for (int k = wv * RPI + h; k < na; k += step) {
            const double re = plane[k * COLS + c], im = plane[cells + k * COLS + c];
            const size_t q = (size_t)((unsigned)k * (unsigned)n + (unsigned)j);
            if constexpr (sizeof(T) == 4) reinterpret_cast<float2*>(Tb)[q] = make_float2((float)re, (float)im);
            else {
                typedef double ssq_d2v __attribute__((ext_vector_type(2)));
                const ssq_d2v v = {re, im};
                __builtin_nontemporal_store(v, reinterpret_cast<ssq_d2v*>(Tb) + q);
            }
        }
    }
}

// ------------------------------------------------- the routing rule (ssq_reassign_route, include/ssq_hip.h)
// Which kernel and build launch_accumulate runs for a shape: the one place that decides, no device call. `real_bytes` is
// sizeof(T); a cell of the ordered tiles is a complex<T>, a cell of the unordered float64 tile 16 bytes for both types.
struct ReassignRoute { int kernel, cols, wavefronts; };

// accumulate_f64_kernel's columns per tile: rows of at least 128 bytes of data per tile, two or more workgroups per CU
// when the tile allows; 0 = the tile does not fit the LDS
static int f64_tile_cols(size_t real_bytes, int64_t na) {
    for (int cols = 32; cols >= 16; cols >>= 1)
        if ((size_t)na * cols * 16 <= LDS_CAP / 2) return cols;
    // (float64 data, 512 rows: 16 columns in one workgroup per CU 4.3 ms, 8 columns in two 4.9 ms)
    if ((size_t)na * 16 * 16 <= LDS_CAP) return 16;
    if (real_bytes == 8 && (size_t)na * 8 * 16 <= LDS_CAP) return 8;
    return 0;
}

static ReassignRoute reassign_route(size_t real_bytes, int binsrc, int64_t na, int64_t n, bool ordered, bool want_kmap) {
    const size_t cell = 2 * real_bytes;
    const bool small = (size_t)na * (size_t)n < ((size_t)1 << 31);     // 32-bit offsets inside the fast kernels
    if (binsrc == BIN_FROM_KIDX) {
        // known bins: the unordered float64 tile (see accumulate_f64_kernel) unless the caller
        // asked for the ordered sums or wants the bin map back
        const int cols = f64_tile_cols(real_bytes, na);
        if (!ordered && !want_kmap && cols && small) return {SSQ_REASSIGN_F64, cols, 8};
    }
    // the DPP-combined, double-buffered kernel: U row batches in flight, RL row-lanes x 64 / RL columns per wavefront,
    // TC-column tiles
    if ((size_t)na * 16 * cell <= LDS_CAP && small) {
        // Row batches in flight per lane. Measured (config 2, float32), 16 row-lanes:
        // U = 2: 257 us, 3: 263, 4: 259, 8: 278; 8 row-lanes: U = 1: 314, 2: 246, 3: 240,
        // 4: 243, 8: 267 -- the resident wavefronts cover most of the latency, and a
        // deep prefetch spreads each wavefront's requests over more DRAM pages.
        // float32: 8 row-lanes x 8 columns per wavefront, 2 wavefronts per 16-column tile (240 us
        // at config 2 vs 250 with 16 row-lanes); float64: 16 row-lanes x 4 columns, 4 wavefronts
        // (config 5: 22.7 vs 23.6 ms).
        if (real_bytes == 4) {
            // 32-column tiles of four 8-lane wavefronts (256-byte row segments per workgroup,
            // 2 workgroups per CU): 232 us at config 2 vs 240 with 16-column tiles (64-column
            // tiles, one workgroup per CU: 231)
            if ((size_t)na * 32 * cell <= LDS_CAP / 2) return {SSQ_REASSIGN_TILE16, 32, 4};
            return {SSQ_REASSIGN_TILE16, 16, 2};
        }
        return {SSQ_REASSIGN_TILE16, 16, 4};
    }
    // larger `na` (or 2^31 points and more): one wavefront per tile, the tile shrunk before giving up on LDS
    if ((size_t)na * 16 * cell <= LDS_CAP / 2) return {SSQ_REASSIGN_TILE, 16, 1};
    if ((size_t)na * 8 * cell <= LDS_CAP / 2) return {SSQ_REASSIGN_TILE, 8, 1};
    if ((size_t)na * 16 * cell <= LDS_CAP) return {SSQ_REASSIGN_TILE, 16, 1};
    if ((size_t)na * 8 * cell <= LDS_CAP) return {SSQ_REASSIGN_TILE, 8, 1};
    if ((size_t)na * 4 * cell <= LDS_CAP) return {SSQ_REASSIGN_TILE, 4, 1};
    return {SSQ_REASSIGN_GLOBAL, 1, 4};
}

template <typename T, bool CST64>
static int launch_accumulate_f64(const void* Wx, const void* kidx, void* Tx, const void* cst,
                                 const SsqParams& sp, int64_t batch, int64_t na, int64_t n,
                                 int cols, hipStream_t stream) {
    constexpr int NW = 8, U = 4;                   // wavefronts per tile, rows in flight per lane
    const size_t lds = (size_t)na * cols * 16;
    dim3 grid((unsigned)(((n + cols - 1) / cols + 7) / 8 * 8), (unsigned)batch);
    auto launch = [&](auto c) -> int {
        return launch_lds(accumulate_f64_kernel<T, CST64, decltype(c)::value, NW, U>, grid, dim3(64 * NW), lds, stream,
                          (const T*)Wx, (const unsigned short*)kidx, (T*)Tx, cst, (int)sp.cst_uniform, (int)na, (int)n);
    };
    if (cols == 32) return launch(int_c<32>{});
    if (cols == 16) return launch(int_c<16>{});
    if constexpr (sizeof(T) == 8) return launch(int_c<8>{});    // (8 columns: float64 data only, see f64_tile_cols)
    return 0;
}

// ---------------------------------------------- accumulate, global fallback
// one thread per time column, serial over rows, Tx (pre-zeroed) updated in place.
template <typename T, int BINSRC, bool STFT, bool CST64>
__global__ __launch_bounds__(256) void accumulate_global_kernel(
    const T* __restrict__ Wx, const void* __restrict__ src, const T* __restrict__ Sfs,
    T* __restrict__ Tx, const void* __restrict__ cst, SsqParams sp, int64_t na, int64_t n,
    int32_t* __restrict__ kmap) {
    using TM = Term<T, CST64>;
    using w_t = typename TM::wtype;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t base = (int64_t)blockIdx.y * na * n;
    const int64_t omax = na - 1;
    for (int64_t i = 0; i < na; ++i) {
        int64_t q = base + i * n + j;
        T c = Wx[2 * q], d = Wx[2 * q + 1];
        SideVal<T, BINSRC> sv;
        sv.load(src, q, i, j, na);
        int64_t k = point_bin<T, BINSRC, STFT>(c, d, sv, i, Sfs, sp, omax);
        if (kmap) kmap[q] = (int32_t)k;
        if (k < 0) continue;
        T* o = Tx + 2 * (base + k * n + j);
        const T ore = o[0], oim = o[1];
        const w_t w = ((const w_t*)cst)[i];
        o[0] = TM::fold(ore, TM::make(c, w)); o[1] = TM::fold(oim, TM::make(d, w));
    }
}

template <typename T, int BINSRC, bool STFT, bool CST64>
static int launch_accumulate_t(const void* Wx, const void* src, const void* Sfs, void* Tx,
                               const void* cst, const SsqParams& sp, int64_t batch,
                               int64_t na, int64_t n, int32_t* kmap, hipStream_t stream) {
    const size_t cell = 2 * sizeof(T);
    const ReassignRoute route = reassign_route(sizeof(T), BINSRC, na, n, reassign_ordered(), kmap != nullptr);
    if constexpr (BINSRC == BIN_FROM_KIDX) {
        if (route.kernel == SSQ_REASSIGN_F64)
            return launch_accumulate_f64<T, CST64>(Wx, src, Tx, cst, sp, batch, na, n, route.cols, stream);
    }
    auto launch_tile = [&](auto tc) -> int {
        constexpr int TC = decltype(tc)::value;
        return launch_lds(accumulate_tile_kernel<T, BINSRC, STFT, CST64, TC>, dim3((unsigned)((n + TC - 1) / TC), (unsigned)batch),
                          dim3(64), (size_t)na * TC * cell, stream, (const T*)Wx, src, (const T*)Sfs, (T*)Tx, cst, sp, na, n,
                          kmap);
    };
    auto launch_tile16 = [&](auto u, auto wps, auto rl, auto tc) -> int {
        constexpr int U = decltype(u)::value, WPS = decltype(wps)::value, RL = decltype(rl)::value, TC = decltype(tc)::value;
        return launch_lds(accumulate_tile16_kernel<T, BINSRC, STFT, CST64, U, WPS, RL, TC>,
                          dim3((unsigned)(((n + TC - 1) / TC + 7) / 8 * 8), (unsigned)batch), dim3(64 * (TC / (64 / RL))),
                          (size_t)na * TC * cell, stream, (const T*)Wx, src, (const T*)Sfs, (T*)Tx, cst, sp, na, n, kmap);
    };
    if (route.kernel == SSQ_REASSIGN_TILE16) {
        if constexpr (sizeof(T) == 4) {
            if (route.cols == 32) return launch_tile16(int_c<3>{}, int_c<2>{}, int_c<8>{}, int_c<32>{});
            return launch_tile16(int_c<3>{}, int_c<2>{}, int_c<8>{}, int_c<16>{});
        } else {
            return launch_tile16(int_c<4>{}, int_c<4>{}, int_c<16>{}, int_c<16>{});
        }
    }
    if (route.kernel == SSQ_REASSIGN_TILE) {
        if (route.cols == 16) return launch_tile(int_c<16>{});
        if (route.cols == 8) return launch_tile(int_c<8>{});
        return launch_tile(int_c<4>{});
    }
    SSQ_CHECK_HIP(hipMemsetAsync(Tx, 0, (size_t)batch * na * n * cell, stream));
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)batch);
    hipLaunchKernelGGL((accumulate_global_kernel<T, BINSRC, STFT, CST64>), grid, dim3(256), 0,
                       stream, (const T*)Wx, src, (const T*)Sfs, (T*)Tx, cst, sp, na, n, kmap);
    SSQ_LAUNCH_CHECK();
    return 0;
}

template <typename T, int BINSRC>
static int launch_accumulate_b(const void* Wx, const void* src, const void* Sfs, void* Tx,
                               const void* cst, const SsqParams& sp, int64_t batch,
                               int64_t na, int64_t n, int32_t* kmap, hipStream_t stream) {
    return dispatch_bool(sp.cst_f64 != 0, [&](auto c) {
        return dispatch_bool(Sfs != nullptr, [&](auto st) {
            // (a float64 weight vector changes the product for float32 data only: float64 data multiplies in float64
            // anyway; Sfs is read when the bins come from dWx only)
            constexpr bool C64 = decltype(c)::value && sizeof(T) == 4;
            constexpr bool STFT = decltype(st)::value && BINSRC == BIN_FROM_DWX;
            return launch_accumulate_t<T, BINSRC, STFT, C64>(Wx, src, STFT ? Sfs : nullptr, Tx, cst, sp, batch, na, n, kmap,
                                                             stream);
        });
    });
}

int launch_accumulate(int dtype, int binsrc, const void* Wx, const void* src, const void* Sfs,
                      void* Tx, const void* cst, const SsqParams& sp, int64_t batch, int64_t na,
                      int64_t n, int32_t* kmap, hipStream_t stream) {
    SSQ_REQUIRE(na >= 1 && n >= 1 && batch >= 1, "accumulate: empty shape (%lld, %lld, %lld)",
                (long long)batch, (long long)na, (long long)n);
    SSQ_REQUIRE(batch <= 65535, "accumulate: batch %lld > 65535", (long long)batch);
    SSQ_REQUIRE(binsrc != BIN_FROM_KIDX || na < 65535, "bin map needs na < 65535");
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        switch (binsrc) {
            case BIN_FROM_DWX: return launch_accumulate_b<T, BIN_FROM_DWX>(Wx, src, Sfs, Tx, cst, sp, batch, na, n, kmap, stream);
            case BIN_FROM_W: return launch_accumulate_b<T, BIN_FROM_W>(Wx, src, Sfs, Tx, cst, sp, batch, na, n, kmap, stream);
            default: return launch_accumulate_b<T, BIN_FROM_KIDX>(Wx, src, Sfs, Tx, cst, sp, batch, na, n, kmap, stream);
        }
    });
}

// ------------------------------------------------- iterated frequency map + accumulate (ssq_multi_squeeze)
#include "ssq_multi_squeeze.inl"

// ------------------------------------------------- adjoint of the reassignment
// The bins are integers, piecewise constant in the data: with them held fixed Tx is linear in Wx and its adjoint is a
// gather, gWx[i][j] (+)= cst[i] * gTx[k(i, j)][j] (0 below gamma), k from the forward's own point math. Reads run along
// j; the product is the forward's (float32 data with a float64 weight: formed in double, rounded once).
template <typename T, bool STFT, bool CST64>
__global__ __launch_bounds__(256) void ssqueeze_adjoint_kernel(
    const T* __restrict__ Wx, const T* __restrict__ dWx, const T* __restrict__ Sfs, const T* __restrict__ gTx,
    T* __restrict__ gWx, const void* __restrict__ cst, SsqParams sp, int64_t batch, int64_t na, int64_t n,
    int accumulate) {
    using TM = Term<T, CST64>;
    using w_t = typename TM::wtype;
    const int64_t total = batch * na * n, omax = na - 1;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q / (na * n), i = (q - b * na * n) / n, j = q - (b * na + i) * n;
        const T c = Wx[2 * q], d = Wx[2 * q + 1];
        SideVal<T, BIN_FROM_DWX> sv;
        sv.load(dWx, q, i, j, na);
        const int64_t k = point_bin<T, BIN_FROM_DWX, STFT>(c, d, sv, i, Sfs, sp, omax);
        T gr = T(0), gi = T(0);
        if (k >= 0) {
            const T* g = gTx + 2 * ((b * na + k) * n + j);
            const w_t w = ((const w_t*)cst)[i];
            gr = (T)TM::make(g[0], w); gi = (T)TM::make(g[1], w);
        }
        if (accumulate) { gr = gWx[2 * q] + gr; gi = gWx[2 * q + 1] + gi; }
        gWx[2 * q] = gr; gWx[2 * q + 1] = gi;
    }
}

// ------------------------------------------------------------------ phase
template <typename T, bool STFT>
__global__ __launch_bounds__(256) void phase_kernel(const T* __restrict__ Wx,
                                                    const T* __restrict__ dWx,
                                                    const T* __restrict__ Sfs, T* __restrict__ w,
                                                    int64_t na, int64_t n, int64_t total,
                                                    double gamma) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total;
         q += (int64_t)gridDim.x * blockDim.x) {
        T c = Wx[2 * q], d = Wx[2 * q + 1];
        // the two-step path thresholds with `abs(Wx) < gamma`, gamma in the data dtype
        if (mag_lt(c, d, (T)gamma)) { w[q] = (T)INFINITY; continue; }
        double r = phase_ratio(dWx[2 * q], dWx[2 * q + 1], c, d);
        if constexpr (STFT) {
            int64_t i = (q / n) % na;
            w[q] = (T)fabs((double)Sfs[i] - r);
        } else {
            w[q] = (T)fabs(r);
        }
    }
}

// ------------------------------------------------- second-order phase (STFT)
// One point of ssq_stft2_phase (include/ssq_hip.h states the map): g, d, dd, t, td are the
// transforms taken with the windows g, g' fs, g'' fs^2, tau g, tau g' fs. The second-order estimate and both thresholds
// are float64 for both dtypes. A point that falls back carries phase_kernel's w bit for bit: the first-order term through
// phase_ratio on the stored values -- for float32 data its float32 numerator and |Vg|^2, the reference's arithmetic --
// so that chirp_tol = inf is phase_stft. Everything is computed and the thresholds select at the end: a point below
// gamma may carry NaN on the way, never in the result.
// Im(P / Q) by Smith's division
__device__ __forceinline__ double smith_im(double pr, double pi, double qr, double qi) {
    const bool wide = fabs(qr) >= fabs(qi);
    const double rat = wide ? qi / qr : qr / qi;
    const double scl = wide ? qr + qi * rat : qr * rat + qi;
    return (wide ? pi - pr * rat : pi * rat - pr) / scl;
}

template <typename T>
__device__ __forceinline__ T stft2_point(T g_re, T g_im, T d_re, T d_im, double ddr, double ddi, double tr, double ti,
                                         double tdr, double tdi, double sfs, double gamma, double chirp_tol) {
    const double gr = g_re, gi = g_im, dr = d_re, di = d_im;
    const double m2 = gr * gr + gi * gi;
    const double w1 = sfs - phase_ratio(dr, di, gr, gi);
    const double w1_fallback = sizeof(T) == 4 ? sfs - phase_ratio(d_re, d_im, g_re, g_im) : w1;
    // num = Vddg Vg - Vdg^2,  den = Vtg Vdg - Vtdg Vg
    const double nr = (ddr * gr - ddi * gi) - (dr * dr - di * di);
    const double ni = (ddr * gi + ddi * gr) - (dr * di + di * dr);
    const double er = (tr * dr - ti * di) - (tdr * gr - tdi * gi);
    const double ei = (tr * di + ti * dr) - (tdr * gi + tdi * gr);
    // Im(P / Q), P = num Vtg, Q = den Vg, by Smith's division (no |Q|^2: float64 data may be tiny)
    const double pr = nr * tr - ni * ti, pi = nr * ti + ni * tr;
    const double qr = er * gr - ei * gi, qi = er * gi + ei * gr;
    const double im = smith_im(pr, pi, qr, qi);
    const bool second = phase2_abs(er, ei, T(0)) > chirp_tol * m2;
    double w = fabs(second ? w1 - im / SSQ_TWO_PI : w1_fallback);
    if (phase2_abs(gr, gi, T(0)) < gamma) w = (double)INFINITY;
    return (T)w;
}

// (Phase2Vec, the 16 bytes of a complex plane, and phase2_abs: ssq_reassign_dev.h)
// Streaming map over the flat (batch, rows, n) index; a thread takes PTS adjacent points per step -- one 16-byte load
// per plane (VEC; the host checks the alignment) or one point with element loads. The row of a point, for Sfs, comes
// from one 32-bit division per step; the second point of a pair may begin the next row.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void stft2_phase_kernel(
    const T* __restrict__ Vg, const T* __restrict__ Vdg, const T* __restrict__ Vddg, const T* __restrict__ Vtg,
    const T* __restrict__ Vtdg, const T* __restrict__ Sfs, T* __restrict__ w, int64_t rows, int64_t n,
    int64_t total, double gamma, double chirp_tol) {
    constexpr int PTS = VEC ? Phase2Vec<T>::PTS : 1;
    const int64_t steps = (total + PTS - 1) / PTS;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < steps; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = s * PTS;
        const unsigned row = (unsigned)q / (unsigned)n;       // (the host guarantees total < 2^32)
        const int64_t i = (int64_t)(row % (unsigned)rows), j = (int64_t)((unsigned)q - row * (unsigned)n);
        if constexpr (PTS == 1) {
            w[q] = stft2_point<T>(Vg[2 * q], Vg[2 * q + 1], Vdg[2 * q], Vdg[2 * q + 1], Vddg[2 * q], Vddg[2 * q + 1],
                                  Vtg[2 * q], Vtg[2 * q + 1], Vtdg[2 * q], Vtdg[2 * q + 1], (double)Sfs[i], gamma,
                                  chirp_tol);
        } else if (q + PTS <= total) {
            using load_t = typename Phase2Vec<T>::load_t;
            const load_t g = reinterpret_cast<const load_t*>(Vg)[s], d = reinterpret_cast<const load_t*>(Vdg)[s],
                         dd = reinterpret_cast<const load_t*>(Vddg)[s], t = reinterpret_cast<const load_t*>(Vtg)[s],
                         td = reinterpret_cast<const load_t*>(Vtdg)[s];
            const int64_t i1 = j + 1 < n ? i : (i + 1 < rows ? i + 1 : 0);
            typename Phase2Vec<T>::store_t o;
            o.x = stft2_point<T>(g.x, g.y, d.x, d.y, dd.x, dd.y, t.x, t.y, td.x, td.y, (double)Sfs[i], gamma, chirp_tol);
            o.y = stft2_point<T>(g.z, g.w, d.z, d.w, dd.z, dd.w, t.z, t.w, td.z, td.w, (double)Sfs[i1], gamma, chirp_tol);
            reinterpret_cast<typename Phase2Vec<T>::store_t*>(w)[s] = o;
        } else {                                        // an odd total: the last point on its own
            w[q] = stft2_point<T>(Vg[2 * q], Vg[2 * q + 1], Vdg[2 * q], Vdg[2 * q + 1], Vddg[2 * q], Vddg[2 * q + 1],
                                  Vtg[2 * q], Vtg[2 * q + 1], Vtdg[2 * q], Vtdg[2 * q + 1], (double)Sfs[i], gamma,
                                  chirp_tol);
        }
    }
}

// -------------------------------------------------- second-order phase (CWT)
// One point of ssq_cwt2_phase (include/ssq_hip.h states the map): g, d, wd, dwd, d3 are W, dW,
// Wd, dWd, dW3; r = scale / fs of the point's row and ri = 1 / r. The constants -1j r and 1j / r are a swap, a sign and a
// real product: T = -1j r Wd, dT = -1j r dWd, ddW = (1j / r) dW3. Types and selects as in stft2_point; the gamma test is
// phase_kernel's own (mag_lt on the stored values, gamma in the data dtype) and the fallback its phase_ratio, so that
// chirp_tol = inf is ssq_phase_cwt bit for bit, infinities included.
template <typename T>
__device__ __forceinline__ T cwt2_point(T g_re, T g_im, T d_re, T d_im, double wdr, double wdi, double dwdr, double dwdi,
                                        double d3r, double d3i, double r, double ri, double gamma, double chirp_tol) {
    const double gr = g_re, gi = g_im, dr = d_re, di = d_im;
    const double tr = r * wdi, ti = -(r * wdr);
    const double sr = gr + r * dwdi, si = gi - r * dwdr;              // W + dT
    const double ddr = -(ri * d3i), ddi = ri * d3r;
    const double m2 = gr * gr + gi * gi;
    const double w1 = phase_ratio(dr, di, gr, gi);
    const double w1_fallback = sizeof(T) == 4 ? phase_ratio(d_re, d_im, g_re, g_im) : w1;
    // den = W (W + dT) - T dW,  num = W ddW - dW^2
    const double er = (gr * sr - gi * si) - (tr * dr - ti * di);
    const double ei = (gr * si + gi * sr) - (tr * di + ti * dr);
    const double nr = (gr * ddr - gi * ddi) - (dr * dr - di * di);
    const double ni = (gr * ddi + gi * ddr) - (dr * di + di * dr);
    // Im(P / Q), P = num T, Q = den W (no |Q|^2: float64 data may be tiny)
    const double pr = nr * tr - ni * ti, pi = nr * ti + ni * tr;
    const double qr = er * gr - ei * gi, qi = er * gi + ei * gr;
    const double im = smith_im(pr, pi, qr, qi);
    const bool second = phase2_abs(er, ei, T(0)) > chirp_tol * m2;
    double w = fabs(second ? w1 - im / SSQ_TWO_PI : w1_fallback);
    if (mag_lt(g_re, g_im, (T)gamma)) w = (double)INFINITY;
    return (T)w;
}

// Streaming map over the flat (batch, na, n) index; a thread takes PTS adjacent points per step, as stft2_phase_kernel
// does -- one 16-byte load per plane (VEC; the host checks the alignment) or one point with element loads. `rtab`:
// (na, 2) float64, scale / fs of a row and its reciprocal, made by the host entry. The row is per point: with n odd the
// two complex64 points of one load belong to different rows. A thread divides once, for its first point; from then on
// its (row, column) advance by the grid's constant stride (no division, and no reciprocal kept in registers, per step).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) SSQ_WAVES_PER_EU(7, 8) void cwt2_phase_kernel(
    const T* __restrict__ W, const T* __restrict__ dW, const T* __restrict__ Wd, const T* __restrict__ dWd,
    const T* __restrict__ dW3, const double* __restrict__ rtab, T* __restrict__ w, int64_t na, int64_t n, int64_t total,
    double gamma, double chirp_tol) {
    constexpr int PTS = VEC ? Phase2Vec<T>::PTS : 1;
    const int64_t steps = (total + PTS - 1) / PTS;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= steps) return;
    // (the host guarantees total < 2^32; the grid has at most 2^21 threads)
    const unsigned un = (unsigned)n, una = (unsigned)na, dq = (unsigned)stride * PTS;
    const unsigned dj = dq % un, di = (dq / un) % una;
    unsigned i, j;
    {
        const unsigned row = (unsigned)(s * PTS) / un;
        i = row % una; j = (unsigned)(s * PTS) - row * un;
    }
    for (; s < steps; s += stride) {
        const int64_t q = s * PTS;
        const double r = rtab[2 * i], ri = rtab[2 * i + 1];
        if constexpr (PTS == 2) {
            if (q + PTS <= total) {
                using load_t = typename Phase2Vec<T>::load_t;
                const load_t g = reinterpret_cast<const load_t*>(W)[s], d = reinterpret_cast<const load_t*>(dW)[s],
                             wd = reinterpret_cast<const load_t*>(Wd)[s], dwd = reinterpret_cast<const load_t*>(dWd)[s],
                             d3 = reinterpret_cast<const load_t*>(dW3)[s];
                const unsigned i1 = j + 1 < un ? i : (i + 1 < una ? i + 1 : 0);
                const double r1 = rtab[2 * i1], ri1 = rtab[2 * i1 + 1];
                typename Phase2Vec<T>::store_t o;
                o.x = cwt2_point<T>(g.x, g.y, d.x, d.y, wd.x, wd.y, dwd.x, dwd.y, d3.x, d3.y, r, ri, gamma, chirp_tol);
                o.y = cwt2_point<T>(g.z, g.w, d.z, d.w, wd.z, wd.w, dwd.z, dwd.w, d3.z, d3.w, r1, ri1, gamma, chirp_tol);
                reinterpret_cast<typename Phase2Vec<T>::store_t*>(w)[s] = o;
            } else {                                    // an odd total: the last point on its own
                w[q] = cwt2_point<T>(W[2 * q], W[2 * q + 1], dW[2 * q], dW[2 * q + 1], Wd[2 * q], Wd[2 * q + 1],
                                     dWd[2 * q], dWd[2 * q + 1], dW3[2 * q], dW3[2 * q + 1], r, ri, gamma, chirp_tol);
            }
        } else if constexpr (VEC) {                     // float64: a point is 16 bytes
            using load_t = typename Phase2Vec<T>::load_t;
            const load_t g = reinterpret_cast<const load_t*>(W)[q], d = reinterpret_cast<const load_t*>(dW)[q],
                         wd = reinterpret_cast<const load_t*>(Wd)[q], dwd = reinterpret_cast<const load_t*>(dWd)[q],
                         d3 = reinterpret_cast<const load_t*>(dW3)[q];
            w[q] = cwt2_point<T>(g.x, g.y, d.x, d.y, wd.x, wd.y, dwd.x, dwd.y, d3.x, d3.y, r, ri, gamma, chirp_tol);
        } else {
            w[q] = cwt2_point<T>(W[2 * q], W[2 * q + 1], dW[2 * q], dW[2 * q + 1], Wd[2 * q], Wd[2 * q + 1], dWd[2 * q],
                                 dWd[2 * q + 1], dW3[2 * q], dW3[2 * q + 1], r, ri, gamma, chirp_tol);
        }
        // (j + dj mod n and i + di + carry mod na, written so that nothing passes 2^32: n or na may be near it)
        const unsigned carry = j >= un - dj, di1 = di + carry;
        j = carry ? j - (un - dj) : j + dj;
        i = i >= una - di1 ? i - (una - di1) : i + di1;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void replace_under_abs_kernel(T* __restrict__ w,
                                                                const T* __restrict__ ref,
                                                                int64_t total, double value,
                                                                T replacement) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total;
         q += (int64_t)gridDim.x * blockDim.x)
        if (mag_of(ref[2 * q], ref[2 * q + 1]) < value) w[q] = replacement;
}

// ---------------------------------------------------------------- framing
template <typename T>
__global__ __launch_bounds__(256) void buffer_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                     int64_t n_x, int64_t seg_len, int64_t n_segs,
                                                     int64_t hop, int64_t s20, int64_t s21,
                                                     int modulated, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        int64_t c = t % n_segs, r = (t / n_segs) % seg_len, b = t / (n_segs * seg_len);
        int64_t start = hop * c, s;
        if (!modulated) s = start + r;
        else if (r < s20) s = start + s21 + r;
        else s = start + (r - s20);
        out[t] = x[b * n_x + s];
    }
}

// ---------------------------------------------------------------- padding
// (the extension rule, pad_source: ssq_common.h, with its transpose)
template <typename T>
__global__ __launch_bounds__(256) void pad_kernel(const T* __restrict__ x, T* __restrict__ out,
                                                  int64_t n, int64_t n1, int64_t m, int padtype,
                                                  int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * blockDim.x) {
        int64_t b = t / m, p = t % m;
        int64_t s = pad_source(p - n1, n, padtype);
        out[t] = s < 0 ? T(0) : x[b * n + s];
    }
}

// Either second-order map: its kernel's 16-byte and element instances, its planes and its row table
template <typename T, typename Tab, typename K>
static void launch_phase2(K vec_kernel, K element_kernel, const void* const (&planes)[5], const Tab* tab, void* w,
                          int64_t rows, int64_t n, int64_t total, double gamma, double chirp_tol, hipStream_t stream) {
    constexpr int PTS = Phase2Vec<T>::PTS;
    // 16-byte loads need every plane on a 16-byte boundary (a caller's offset pointer need not be), the store of a
    // step's results its own width
    bool vec = ((uintptr_t)w % (PTS * sizeof(T))) == 0;
    for (const void* p : planes) vec = vec && ((uintptr_t)p % 16) == 0;
    hipLaunchKernelGGL(vec ? vec_kernel : element_kernel, dim3(stream_grid(vec ? (total + PTS - 1) / PTS : total)),
                       dim3(256), 0, stream, (const T*)planes[0], (const T*)planes[1], (const T*)planes[2],
                       (const T*)planes[3], (const T*)planes[4], tab, (T*)w, rows, n, total, gamma, chirp_tol);
}

}  // namespace ssq

using namespace ssq;

// ======================================================================= C ABI
// the build's stamp: ssqueezepy_amd/build.py links a strong definition (the last commit that touched
// csrc/ or include/) over this one
extern "C" __attribute__((weak)) const char ssq_build_sha_value[] = "unknown";

extern "C" {

const char* ssq_build_sha(void) { return ssq_build_sha_value; }
int ssq_version(void) { return 120; }   // 120: ssq_time_reassign_cwt, ssq_time_reassign_cwt_tile; 119: ssq_multi_squeeze_cwt, ssq_multi_squeeze_cwt_max_rows, ssq_multi_squeeze_cwt_tile; 118: ssq_reassign_route, ssq_indexed_sum_bins; 117: ssq_reassign_cwt, ssq_reassign_cwt_tile; 116: ssq_stft_generic_shape; 115: ssq_reassign2d, ssq_reassign2d_tile; 114: ssq_multi_squeeze, ssq_multi_squeeze_max_rows; 113: ssq_time_reassign, ssq_time_reassign_segment, ssq_time_reassign_max_dmax; 112: ssq_conceft_cwt; 111: ssq_conceft; 110: ssq_cwt2_phase; 109: ssq_stft2_phase; 108: ssq_cwt_adjoint; 107: ssq_istft_batch, ssq_istft_adjoint, ssq_istft_algo, ssq_colsum_adjoint, ssq_band_colsum_batch, ssq_band_colsum_adjoint; 106: ssq_stft_adjoint, ssq_ssqueeze_adjoint; 105: ssq_cwt_plan_tile_kernel; 104: ssq_build_sha, ssq_cwt_plan_set_bin_dump; 103: ssq_ridge_*_batch; 102: ssq_cwt_plan_tile_cols; 101: ssq_cwt_blocks_desc.classes has 5 columns (analytic classes)
const char* ssq_last_error(void) { return g_last_error.c_str(); }

int ssq_device_count(int* count) {
    SSQ_REQUIRE(count, "ssq_device_count: null pointer");
    SSQ_CHECK_HIP(hipGetDeviceCount(count));
    return 0;
}
int ssq_set_device(int device) { SSQ_CHECK_HIP(hipSetDevice(device)); return 0; }

int ssq_device_info(int device, char* name, int len, int* cus, int64_t* hbm_bytes) {
    hipDeviceProp_t prop;
    SSQ_CHECK_HIP(hipGetDeviceProperties(&prop, device));
    if (name && len > 0) { strncpy(name, prop.gcnArchName, len - 1); name[len - 1] = 0; }
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return 0;
}

int ssq_malloc(void** ptr, int64_t bytes) {
    SSQ_REQUIRE(ptr && bytes >= 0, "ssq_malloc: bad arguments");
    SSQ_CHECK_HIP(hipMalloc(ptr, (size_t)(bytes > 0 ? bytes : 1)));
    return 0;
}
int ssq_free(void* ptr) { SSQ_CHECK_HIP(hipFree(ptr)); return 0; }
int ssq_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream) {
    SSQ_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, as_stream(stream)));
    return 0;
}
int ssq_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream) {
    SSQ_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, as_stream(stream)));
    return 0;
}
int ssq_memset(void* dst, int value, int64_t bytes, void* stream) {
    SSQ_CHECK_HIP(hipMemsetAsync(dst, value, (size_t)bytes, as_stream(stream)));
    return 0;
}
int ssq_stream_synchronize(void* stream) {
    SSQ_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    return 0;
}

int ssq_phase_cwt(int dtype, const void* Wx, const void* dWx, void* w, int64_t batch, int64_t na,
                  int64_t n, double gamma, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Wx && dWx && w, "ssq_phase_cwt: null pointer");
    int64_t total = batch * na * n;
    if (total == 0) return 0;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((phase_kernel<T, false>), dim3(stream_grid(total)), dim3(256), 0, as_stream(stream),
                           (const T*)Wx, (const T*)dWx, (const T*)nullptr, (T*)w, na, n, total, gamma);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_phase_stft(int dtype, const void* Sx, const void* dSx, const void* Sfs, void* w,
                   int64_t batch, int64_t na, int64_t n, double gamma, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Sx && dSx && Sfs && w, "ssq_phase_stft: null pointer");
    int64_t total = batch * na * n;
    if (total == 0) return 0;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((phase_kernel<T, true>), dim3(stream_grid(total)), dim3(256), 0, as_stream(stream),
                           (const T*)Sx, (const T*)dSx, (const T*)Sfs, (T*)w, na, n, total, gamma);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

// What the two second-order entries check alike, in the order they always did (`entry` names the caller in the message)
static int check_phase2(const char* entry, const void* const (&planes)[5], const void* tab, const void* w, int64_t batch,
                        int64_t rows, int min_rows, int64_t n, double chirp_tol) {
    SSQ_REQUIRE(planes[0] && planes[1] && planes[2] && planes[3] && planes[4] && tab && w, "%s: null pointer", entry);
    SSQ_REQUIRE(batch >= 1 && rows >= min_rows && n >= 1, "%s: bad shape (%lld, %lld, %lld): rows >= %d, batch, n >= 1",
                entry, (long long)batch, (long long)rows, (long long)n, min_rows);
    SSQ_REQUIRE(chirp_tol >= 0.0, "%s: chirp_tol must be >= 0 (got %g)", entry, chirp_tol);
    return check_point_count(entry, batch, rows, n);
}

int ssq_stft2_phase(int dtype, const void* Vg, const void* Vdg, const void* Vddg, const void* Vtg, const void* Vtdg,
                    const void* Sfs, void* w, int64_t batch, int64_t rows, int64_t n, double gamma, double chirp_tol,
                    void* stream) {
    if (check_dtype(dtype)) return -1;
    const void* const planes[5] = {Vg, Vdg, Vddg, Vtg, Vtdg};
    if (check_phase2("ssq_stft2_phase", planes, Sfs, w, batch, rows, 2, n, chirp_tol)) return -1;
    if (check_gamma("ssq_stft2_phase", gamma)) return -1;
    const int64_t total = batch * rows * n;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        launch_phase2<T>(stft2_phase_kernel<T, true>, stft2_phase_kernel<T, false>, planes, (const T*)Sfs, w, rows, n, total,
                         gamma, chirp_tol, as_stream(stream));
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

// The rows' r = scale / fs and 1 / r in float64, (na, 2), on the current device: checked on the host, uploaded once per
// (device, contents) and kept
static DeviceTableCache g_cwt2_tables;

static int cwt2_row_table(const double* scales, int64_t na, double fs, const double** out) {
    std::vector<double> rtab((size_t)na * 2);
    for (int64_t i = 0; i < na; ++i) {
        const double r = scales[i] / fs;
        SSQ_REQUIRE(scales[i] > 0.0 && r > 0.0 && r <= DBL_MAX && 1.0 / r > 0.0 && 1.0 / r <= DBL_MAX,
                    "ssq_cwt2_phase: scales[%lld] = %g: scales must be positive (and scale / fs, fs / scale finite)",
                    (long long)i, scales[i]);
        rtab[2 * i] = r; rtab[2 * i + 1] = 1.0 / r;
    }
    return g_cwt2_tables.get(rtab.data(), rtab.size(), out);
}

int ssq_cwt2_phase(int dtype, const void* W, const void* dW, const void* Wd, const void* dWd, const void* dW3,
                   const double* scales, void* w, int64_t batch, int64_t na, int64_t n, double fs, double gamma,
                   double chirp_tol, void* stream) {
    if (check_dtype(dtype)) return -1;
    const void* const planes[5] = {W, dW, Wd, dWd, dW3};
    if (check_phase2("ssq_cwt2_phase", planes, scales, w, batch, na, 1, n, chirp_tol)) return -1;
    SSQ_REQUIRE(fs > 0.0 && fs <= DBL_MAX, "ssq_cwt2_phase: fs must be positive and finite (got %g)", fs);
    const int64_t total = batch * na * n;
    const double* rdev = nullptr;
    if (cwt2_row_table(scales, na, fs, &rdev)) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        launch_phase2<T>(cwt2_phase_kernel<T, true>, cwt2_phase_kernel<T, false>, planes, rdev, w, na, n, total, gamma,
                         chirp_tol, as_stream(stream));
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_ssqueeze(int dtype, const void* Wx, const void* dWx, const void* Sfs, void* Tx,
                 const void* cst, int cst_f64, int64_t batch, int64_t na, int64_t n, double gamma,
                 int grid, const double* params, int flipud, int32_t* kmap, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Wx && dWx && Tx && cst, "ssq_ssqueeze: null pointer");
    SsqParams sp;
    if (fill_params(sp, grid, params, flipud, gamma, cst_f64)) return -1;
    return launch_accumulate(dtype, BIN_FROM_DWX, Wx, dWx, Sfs, Tx, cst, sp, batch, na, n, kmap, as_stream(stream));
}

int ssq_ssqueeze_adjoint(int dtype, const void* Wx, const void* dWx, const void* Sfs, const void* gTx, void* gWx,
                         int accumulate, const void* cst, int cst_f64, int64_t batch, int64_t na, int64_t n,
                         double gamma, int grid, const double* params, int flipud, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Wx && dWx && gTx && gWx && cst, "ssq_ssqueeze_adjoint: null pointer");
    SSQ_REQUIRE(na >= 1 && n >= 1 && batch >= 1, "ssqueeze_adjoint: empty shape (%lld, %lld, %lld)",
                (long long)batch, (long long)na, (long long)n);
    SsqParams sp;
    if (fill_params(sp, grid, params, flipud, gamma, cst_f64)) return -1;
    const dim3 g(stream_grid(batch * na * n));
    hipStream_t s = as_stream(stream);
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return dispatch_bool(cst_f64 != 0, [&](auto c) {
            return dispatch_bool(Sfs != nullptr, [&](auto st) {
                constexpr bool C64 = decltype(c)::value && sizeof(T) == 4;    // (as launch_accumulate_b)
                hipLaunchKernelGGL((ssqueeze_adjoint_kernel<T, decltype(st)::value, C64>), g, dim3(256), 0, s, (const T*)Wx,
                                   (const T*)dWx, (const T*)Sfs, (const T*)gTx, (T*)gWx, cst, sp, batch, na, n, accumulate);
                SSQ_LAUNCH_CHECK();
                return 0;
            });
        });
    });
}

int ssq_indexed_sum(int dtype, const void* Wx, const void* w, void* Tx, const void* cst, int cst_f64,
                    int64_t batch, int64_t na, int64_t n, int grid, const double* params, int flipud,
                    void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Wx && w && Tx && cst, "ssq_indexed_sum: null pointer");
    SsqParams sp;
    if (fill_params(sp, grid, params, flipud, 0.0, cst_f64)) return -1;
    return launch_accumulate(dtype, BIN_FROM_W, Wx, w, nullptr, Tx, cst, sp, batch, na, n, nullptr, as_stream(stream));
}

int ssq_indexed_sum_bins(int dtype, const void* Wx, const void* kidx, void* Tx, const void* cst, int cst_f64,
                         int64_t batch, int64_t na, int64_t n, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Wx && kidx && Tx && cst, "ssq_indexed_sum_bins: null pointer");
    const double no_grid[5] = {0.0, 1.0, 0.0, 0.0, 0.0};        // (the bins are given: no grid is read)
    SsqParams sp;
    if (fill_params(sp, SSQ_GRID_LIN, no_grid, 0, 0.0, cst_f64)) return -1;
    return launch_accumulate(dtype, BIN_FROM_KIDX, Wx, kidx, nullptr, Tx, cst, sp, batch, na, n, nullptr, as_stream(stream));
}

int ssq_reassign_route(int dtype, int binsrc, int64_t na, int64_t n, int ordered, int want_kmap, int* kernel, int* cols,
                       int* wavefronts) {
    if (kernel) *kernel = -1;
    if (cols) *cols = 0;
    if (wavefronts) *wavefronts = 0;
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(binsrc == BIN_FROM_DWX || binsrc == BIN_FROM_W || binsrc == BIN_FROM_KIDX,
                "ssq_reassign_route: binsrc = %d, 0 (dWx), 1 (stored w) or 2 (bin map)", binsrc);
    SSQ_REQUIRE(na >= 1 && n >= 1, "ssq_reassign_route: empty shape (%lld, %lld)", (long long)na, (long long)n);
    SSQ_REQUIRE(binsrc != BIN_FROM_KIDX || na < 65535, "bin map needs na < 65535");
    const ReassignRoute r = reassign_route(dtype == SSQ_F32 ? 4 : 8, binsrc, na, n, ordered != 0, want_kmap != 0);
    if (kernel) *kernel = r.kernel;
    if (cols) *cols = r.cols;
    if (wavefronts) *wavefronts = r.wavefronts;
    return 0;
}

int ssq_multi_squeeze_max_rows(int dtype) {
    if (dtype == SSQ_F32) return (int)msst_tile_rows<float>(MSST_WC);
    return dtype == SSQ_F64 ? (int)msst_tile_rows<double>(MSST_WC) : 0;
}

int ssq_multi_squeeze(int dtype, const void* Sx, const void* w, void* Tx, void* wf, const void* cst, int cst_f64,
                      int64_t batch, int64_t rows, int64_t n, double f0, double df, int64_t n_iter, int interp, int grid,
                      const double* params, int flipud, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(Sx && w && Tx && cst && params, "ssq_multi_squeeze: null pointer");
    SSQ_REQUIRE(batch >= 1 && rows >= 2 && n >= 1, "ssq_multi_squeeze: bad shape (%lld, %lld, %lld): rows >= 2, batch, n >= 1",
                (long long)batch, (long long)rows, (long long)n);
    SSQ_REQUIRE(rows <= ssq_multi_squeeze_max_rows(dtype), "ssq_multi_squeeze: %lld rows, at most %d (a 4-column tile of Tx and w in LDS)",
                (long long)rows, ssq_multi_squeeze_max_rows(dtype));
    if (check_point_count("ssq_multi_squeeze", batch, rows, n)) return -1;
    SSQ_REQUIRE(n_iter >= 1 && n_iter <= MSST_MAX_ITER, "ssq_multi_squeeze: n_iter = %lld, 1 .. %lld", (long long)n_iter,
                (long long)MSST_MAX_ITER);
    SSQ_REQUIRE(interp == 0 || interp == 1, "ssq_multi_squeeze: interp = %d, 0 (nearest row) or 1 (linear)", interp);
    SSQ_REQUIRE(df > 0.0 && df <= DBL_MAX && fabs(f0) <= DBL_MAX,
                "ssq_multi_squeeze: f0 = %g, df = %g: f0 finite, df positive and finite", f0, df);
    SsqParams sp;
    if (fill_params(sp, grid, params, flipud, 0.0, cst_f64, "ssq_multi_squeeze")) return -1;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return dispatch_bool(cst_f64 != 0, [&](auto c) {
            constexpr bool C64 = decltype(c)::value && sizeof(T) == 4;    // (as launch_accumulate_b)
            return launch_multi_squeeze<T, C64>(Sx, w, Tx, wf, cst, sp, batch, rows, n, MsstLinearRows{f0, df}, n_iter,
                                                interp, as_stream(stream));
        });
    });
}

int ssq_multi_squeeze_cwt_max_rows(int dtype) {
    if (dtype == SSQ_F32) return (int)msst_tile_rows<float>(MSST_WC, MsstTableRows::ROW_BYTES);
    return dtype == SSQ_F64 ? (int)msst_tile_rows<double>(MSST_WC, MsstTableRows::ROW_BYTES) : 0;
}

int ssq_multi_squeeze_cwt_tile(int dtype, int64_t rows) {
    if (rows < 2) return 0;
    if (dtype == SSQ_F32) return msst_tile_cols<float, MsstTableRows>(rows);
    return dtype == SSQ_F64 ? msst_tile_cols<double, MsstTableRows>(rows) : 0;
}

// The rows' centre frequencies on the current device: checked on the host, uploaded once per (device, contents), kept
static DeviceTableCache g_msst_cwt_tables;

int ssq_multi_squeeze_cwt(int dtype, const void* Wx, const void* w, void* Tx, void* wf, const void* cst, int cst_f64,
                          const double* fr, int64_t batch, int64_t rows, int64_t n, int64_t n_iter, int interp, int grid,
                          const double* params, int flipud, void* stream) {
    SSQ_REQUIRE(dtype == SSQ_F32 || dtype == SSQ_F64, "ssq_multi_squeeze_cwt: dtype must be SSQ_F32 or SSQ_F64 (got %d)", dtype);
    SSQ_REQUIRE(Wx && w && Tx && cst && fr && params, "ssq_multi_squeeze_cwt: null pointer");
    SSQ_REQUIRE(batch >= 1 && rows >= 2 && n >= 1, "ssq_multi_squeeze_cwt: bad shape (%lld, %lld, %lld): rows >= 2, batch, n >= 1",
                (long long)batch, (long long)rows, (long long)n);
    SSQ_REQUIRE(rows <= ssq_multi_squeeze_cwt_max_rows(dtype),
                "ssq_multi_squeeze_cwt: %lld rows, at most %d (a 4-column tile of Tx and w and the rows' table in LDS)",
                (long long)rows, ssq_multi_squeeze_cwt_max_rows(dtype));
    if (check_point_count("ssq_multi_squeeze_cwt", batch, rows, n)) return -1;
    SSQ_REQUIRE(n_iter >= 1 && n_iter <= MSST_MAX_ITER, "ssq_multi_squeeze_cwt: n_iter = %lld, 1 .. %lld", (long long)n_iter,
                (long long)MSST_MAX_ITER);
    SSQ_REQUIRE(interp == 0 || interp == 1, "ssq_multi_squeeze_cwt: interp = %d, 0 (nearest row) or 1 (linear)", interp);
    const int desc = fr[1] < fr[0];
    for (int64_t i = 0; i < rows; ++i) {
        SSQ_REQUIRE(fabs(fr[i]) <= DBL_MAX, "ssq_multi_squeeze_cwt: fr[%lld] = %g: the rows' frequencies must be finite",
                    (long long)i, fr[i]);
        SSQ_REQUIRE(i == 0 || (desc ? fr[i] < fr[i - 1] : fr[i] > fr[i - 1]),
                    "ssq_multi_squeeze_cwt: fr[%lld] = %g after %g: the rows' frequencies must be strictly monotone",
                    (long long)i, fr[i], fr[i - 1]);
    }
    SsqParams sp;
    if (fill_params(sp, grid, params, flipud, 0.0, cst_f64, "ssq_multi_squeeze_cwt")) return -1;
    const double* fr_dev = nullptr;
    if (g_msst_cwt_tables.get(fr, (size_t)rows, &fr_dev)) return -1;
    const MsstTableRows pos{fr_dev, desc ? fr[rows - 1] : fr[0], desc ? fr[0] : fr[rows - 1], desc, msst_fit_hint(fr, rows),
                            nullptr};
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return dispatch_bool(cst_f64 != 0, [&](auto c) {
            constexpr bool C64 = decltype(c)::value && sizeof(T) == 4;    // (as launch_accumulate_b)
            return launch_multi_squeeze<T, C64>(Wx, w, Tx, wf, cst, sp, batch, rows, n, pos, n_iter, interp,
                                                as_stream(stream));
        });
    });
}

int ssq_replace_under_abs(int dtype, void* w, const void* ref, int64_t count, double value,
                          double replacement, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(w && ref, "ssq_replace_under_abs: null pointer");
    if (count == 0) return 0;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((replace_under_abs_kernel<T>), dim3(stream_grid(count)), dim3(256), 0, as_stream(stream),
                           (T*)w, (const T*)ref, count, value, (T)replacement);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_buffer(int dtype, const void* x, void* out, int64_t batch, int64_t n_x, int64_t seg_len,
               int64_t n_overlap, int modulated, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(x && out, "ssq_buffer: null pointer");
    int64_t hop = seg_len - n_overlap;
    SSQ_REQUIRE(seg_len >= 1 && hop >= 1 && n_x >= seg_len, "ssq_buffer: bad framing (n_x=%lld seg_len=%lld n_overlap=%lld)",
                (long long)n_x, (long long)seg_len, (long long)n_overlap);
    int64_t n_segs = (n_x - seg_len) / hop + 1;
    int64_t s20 = (seg_len + 1) / 2, s21 = (seg_len % 2 == 1) ? s20 - 1 : s20;
    int64_t total = batch * seg_len * n_segs;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((buffer_kernel<T>), dim3(stream_grid(total)), dim3(256), 0, as_stream(stream),
                           (const T*)x, (T*)out, n_x, seg_len, n_segs, hop, s20, s21, modulated, total);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

int ssq_pad_signal(int dtype, const void* x, void* out, int64_t batch, int64_t n, int64_t n1,
                   int64_t n2, int padtype, void* stream) {
    if (check_dtype(dtype)) return -1;
    SSQ_REQUIRE(x && out, "ssq_pad_signal: null pointer");
    SSQ_REQUIRE(padtype >= SSQ_PAD_ZERO && padtype <= SSQ_PAD_WRAP, "unknown padtype %d", padtype);
    int64_t m = n1 + n + n2, total = batch * m;
    if (total == 0) return 0;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pad_kernel<T>), dim3(stream_grid(total)), dim3(256), 0, as_stream(stream),
                           (const T*)x, (T*)out, n, n1, m, padtype, total);
        SSQ_LAUNCH_CHECK();
        return 0;
    });
}

}  // extern "C"

// hipcc (build.py) and the tests' CPU emulator (tests/emu/Makefile, which says SSQ_EMU_UNITS_SPLIT) compile
// ssq_conceft.hip and ssq_time_reassign.hip as units of their own. Only an emulator build from a unit list older than
// the split -- the tests directory of an earlier commit run against these sources -- lacks them and gets them here, so
// that its library still has every entry.
#if !defined(__HIPCC__) && !defined(SSQ_EMU_UNITS_SPLIT)
#include "ssq_conceft.hip"
#include "ssq_time_reassign.hip"
#endif
