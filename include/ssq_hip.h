/*
 * ssq_hip.h -- C ABI of libssq_hip.so, the MI355X (gfx950) engine behind
 * ssqueezepy_amd's cwt() / stft() / ssq_cwt() / ssq_stft().
 *
 * The reference (OverLordGoldDragon/ssqueezepy v0.6.6) has no FFI: its GPU seam is
 * Python-level -- CuPy RawModule kernels launched with raw device pointers on
 * torch's current stream (ssqueezepy/utils/gpu_utils.py:10-21, algos.py:100-105).
 * This header is that seam restated as a C ABI: plain pointers and sizes, no torch
 * or HIP types in the signatures (`stream` is a hipStream_t passed as void*, NULL =
 * the default stream), every entry point asynchronous on its stream, int status
 * returns (0 = ok, <0 = error, text via ssq_last_error()), no exceptions across the
 * boundary. Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *   dtype      SSQ_F32 / SSQ_F64: the *real* type; complex arrays are interleaved
 *              (re, im) pairs of it (what torch.view_as_real gives, algos.py:61-64).
 *   layouts    2-D arrays are row-major (rows = scales / frequency bins,
 *              cols = time); batched arrays put the signal index first.
 *   pointers   every array is dense in the stated order: no strides, no padding between
 *              rows or signals, and the pointer addresses the values themselves (a host
 *              framework's lazy conjugate / negative / broadcast view must be
 *              materialised first). A pointer needs only the alignment of its element:
 *              4 / 8 bytes for real SSQ_F32 / SSQ_F64 data, 8 / 16 bytes for a complex
 *              (re, im) pair, 4 for int32 -- `buf + 1` of an allocation is as good as
 *              `buf`. Kernels that move 16 bytes at a time declare the lower alignment
 *              on the access or test the address and take narrower accesses.
 *   aliasing   no output may overlap an input or another output of the same call. The
 *              exceptions are stated at the entry point: ssq_replace_under_abs works in
 *              place on `w`, ssq_icwt2 uses `Wp` as its workspace and overwrites it,
 *              and ssq_ssqueeze_adjoint with `accumulate` adds to `gWx`. In particular
 *              the reassignments scatter: `Tx` must not be `Wx`, `dWx` or `w`, and a
 *              gradient output must not be the incoming gradient.
 *   ownership  the caller owns every I/O buffer (device memory); plans own their
 *              FFT plans, workspace and the device copy of the filter bank.
 *   threading  one plan per host thread / stream at a time; plans are immutable
 *              after creation except through the documented setters.
 */
#ifndef SSQ_HIP_H
#define SSQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSQ_F32 0
#define SSQ_F64 1

#define SSQ_GRID_LOG 0            /* params: vlmin, dvl                         */
#define SSQ_GRID_LOG_PIECEWISE 1  /* params: vlmin0, vlmin1, dvl0, dvl1, idx1   */
#define SSQ_GRID_LIN 2            /* params: vmin, dv                           */

#define SSQ_PAD_NONE (-1)
#define SSQ_PAD_ZERO 0
#define SSQ_PAD_REFLECT 1
#define SSQ_PAD_SYMMETRIC 2
#define SSQ_PAD_REPLICATE 3
#define SSQ_PAD_WRAP 4

/* ------------------------------------------------------------------ runtime */
int         ssq_version(void);          /* 120 (119: without ssq_time_reassign_cwt; 118: without ssq_multi_squeeze_cwt; 117: without ssq_reassign_route / ssq_indexed_sum_bins; 116: without ssq_reassign_cwt; 115: without ssq_stft_generic_shape; 114: without ssq_reassign2d; 113: without ssq_multi_squeeze; 112: without ssq_time_reassign; 111: without ssq_conceft_cwt; 110: without ssq_conceft; 109: without ssq_cwt2_phase; 108: without ssq_stft2_phase; 107: without ssq_cwt_adjoint; 106: without the batched inverses and their adjoints: ssq_istft_batch / ssq_istft_adjoint / ssq_istft_algo / ssq_colsum_adjoint / ssq_band_colsum_batch / ssq_band_colsum_adjoint; 105: without ssq_stft_adjoint / ssq_ssqueeze_adjoint; 104: without ssq_cwt_plan_tile_kernel; 103: without ssq_build_sha / ssq_cwt_plan_set_bin_dump; 102: without ssq_ridge_*_batch; 101: without ssq_cwt_plan_tile_cols; 100: block classes without the `analytic` column) */
/* The git commit of the device code this library was built from: the last commit that touched
 * ssqueezepy_amd/csrc or include/ ("<sha>-dirty" when the build tree had uncommitted changes there,
 * "unknown" when built outside a git checkout). Measurement records carry it (bench.py, profiles/):
 * evidence and library can be matched without trusting a file name. */
const char* ssq_build_sha(void);
const char* ssq_last_error(void);
int         ssq_device_count(int* count);
int         ssq_set_device(int device);
/* name[0..len) <- gcnArchName of `device`; *cus <- compute-unit count */
int         ssq_device_info(int device, char* name, int len, int* cus,
                            int64_t* hbm_bytes);

/* Raw device-memory helpers for hosts that do not bring their own allocator
 * (the Python layer normally passes torch-owned device pointers instead). */
int ssq_malloc(void** ptr, int64_t bytes);
int ssq_free(void* ptr);
int ssq_memcpy_h2d(void* dst, const void* src, int64_t bytes, void* stream);
int ssq_memcpy_d2h(void* dst, const void* src, int64_t bytes, void* stream);
int ssq_memset(void* dst, int value, int64_t bytes, void* stream);
int ssq_stream_synchronize(void* stream);

/* ---------------------------------------------------- kernel-level seam
 * These are the reference's L2 kernels. All arrays are
 * (batch, na, n) device arrays; `batch` >= 1.
 */

/* w = |Wx| < gamma ? inf : |Im(dWx / Wx)| / 2pi
 * replaces phase_cwt_cpu / phase_cwt_gpu (algos.py:706-781). */
int ssq_phase_cwt(int dtype, const void* Wx, const void* dWx, void* w,
                  int64_t batch, int64_t na, int64_t n, double gamma,
                  void* stream);

/* w = |Sx| < gamma ? inf : |Sfs[i] - Im(dSx / Sx) / 2pi|
 * replaces phase_stft_cpu / phase_stft_gpu (algos.py:784-856). Sfs: (na,) real. */
int ssq_phase_stft(int dtype, const void* Sx, const void* dSx, const void* Sfs,
                   void* w, int64_t batch, int64_t na, int64_t n, double gamma,
                   void* stream);

/* Second-order phase transform of the STFT (ABI 109; Oberlin, Meignen, Perrier 2015; Behera, Meignen, Oberlin 2018;
 * DESIGN.md section 4.5.3 states the definition). Five STFTs of one signal, (batch, rows, n) complex each, taken with the
 * windows g, g' fs, g'' fs^2, tau g and tau g' fs (tau = the window's time axis in seconds, 0 at its centre):
 *   w1  = Sfs[i] - Im(Vdg / Vg) / 2pi                                   first-order estimate, Hz
 *   den = Vtg Vdg - Vtdg Vg
 *   w2  = w1 - Im( (Vddg Vg - Vdg^2) Vtg / (den Vg) ) / 2pi             = Re(w1c - q Vtg / Vg), q the chirp rate
 *   w   = |Vg| < gamma ? inf : |den| > chirp_tol |Vg|^2 ? |w2| : |w1|
 * evaluated per point in float64 for both dtypes (float32 planes are promoted) and rounded once to `dtype`; the
 * fallback |w1| is ssq_phase_stft's value bit for bit (float32 data: its float32 numerator and |Vg|^2).
 * Sfs: (rows,) real; w: (batch, rows, n) real. One streaming pass: every plane read once, w written once. The gamma
 * test is on |Vg| in float64 for both dtypes (ssq_cwt2_phase's is ssq_phase_cwt's). There is no counterpart in the
 * reference. rows >= 2, batch, n >= 1, batch rows n < 2^32, chirp_tol >= 0 (+inf: first order
 * everywhere). */
int ssq_stft2_phase(int dtype, const void* Vg, const void* Vdg, const void* Vddg, const void* Vtg,
                    const void* Vtdg, const void* Sfs, void* w, int64_t batch, int64_t rows, int64_t n,
                    double gamma, double chirp_tol, void* stream);

/* Second-order phase transform of the CWT (ABI 110; Oberlin, Meignen 2017; DESIGN.md section 4.5.4 states the
 * definition). Five planes, (batch, na, n) complex each, from three CWTs of one signal over real banks -- psih the
 * wavelet in the frequency domain, w its argument (scale x radians per sample):
 *   W, dW    Wx, dWx of the bank psih(w)           dW = fs ifft(i xi psih(a xi) xh), the time derivative per second
 *   Wd, dWd  Wx, dWx of the bank psih'(w) = d psih / dw
 *   dW3      dWx of the bank w psih(w)
 * With r = scales[i] / fs (the scale of row i in seconds):
 *   T   = -1j r Wd     dT = -1j r dWd     ddW = (1j / r) dW3        (T: the CWT taken with t psi(t); ddW: d^2 W / dt^2)
 *   den = W (W + dT) - T dW
 *   num = W ddW - dW^2                                               num / den / (2pi j): the chirp rate, Hz/s
 *   w1  = Im(dW / W) / 2pi                                           first-order estimate, Hz
 *   w2  = w1 - Im( num T / (den W) ) / 2pi
 *   w   = |W| < gamma ? inf : |den| > chirp_tol |W|^2 ? |w2| : |w1|
 * evaluated per point in float64 for both dtypes (float32 planes are promoted) and rounded once to `dtype`; the
 * gamma test and the fallback |w1| are ssq_phase_cwt's bit for bit (float32 data: gamma and |W| in float32, the
 * float32 numerator and |W|^2), so chirp_tol = +inf gives ssq_phase_cwt's w. den / W^2 is 1 on a tone and 0 on an
 * impulse, where no chirp rate exists.
 * scales: HOST array of na float64, read before the call returns: the entry checks it and keeps scale / fs and its
 * reciprocal on the device, one small table per (device, fs, scales), the eight most recent. A call whose table exists
 * only enqueues the kernel -- asynchronous like every other entry, and capturable into a graph; the first call with
 * new scales uploads the table synchronously (hipMalloc, hipMemcpy) and must not be made under stream capture;
 * w: (batch, na, n) real. One streaming pass: every plane
 * read once, w written once. No counterpart in the reference. Refused, with w unwritten: batch, na or n < 1,
 * batch na n >= 2^32, chirp_tol < 0 or NaN, fs <= 0 or not finite, a scale <= 0 or not finite. */
int ssq_cwt2_phase(int dtype, const void* W, const void* dW, const void* Wd, const void* dWd, const void* dW3,
                   const double* scales, void* w, int64_t batch, int64_t na, int64_t n, double fs, double gamma,
                   double chirp_tol, void* stream);

/* Multitaper synchrosqueezing, ConceFT (ABI 111; Daubechies, Wang, Wu 2016). J transforms of
 * one signal taken with J orthonormal windows, V_j, and with the windows' derivatives, dV_j -- (batch, rows, n) complex
 * planes each -- are combined into Q projections, each projection is synchrosqueezed, and the results are averaged.
 *   V, dV   HOST arrays of J device pointers
 *   Sfs     (rows,) real `dtype`, device
 *   proj    HOST (Q, J, 2) float64: re, im of r[q][j]; read before the call returns (the entry keeps a device copy per
 *           (device, contents), the eight most recent: a call whose copy exists only enqueues the kernel; the first
 *           call with new contents uploads synchronously and must not be made under stream capture)
 *   Cx      (batch, rows, n): real `dtype` (average = 0) or complex `dtype` (average = 1); overwritten
 * Evaluated in float64 for both dtypes (float32 planes are promoted), no contraction. Per signal b, column c,
 * projection q = 0 .. Q-1, with Tq a column of `rows` float64 complex cells, zero at first:
 *   for i = 0 .. rows-1 (ascending):
 *       Vq  = sum_j r[q][j] * V_j[b,i,c]     from 0, ascending j; each product as (ar*vr - ai*vi, ar*vi + ai*vr);
 *                                            the real and the imaginary sum separate
 *       dVq = the same over dV_j
 *       if hypot(Vq.re, Vq.im) < gamma: continue
 *       w = | Sfs[i] - (dVq.im*Vq.re - dVq.re*Vq.im) / ((Vq.re^2 + Vq.im^2) * 2pi) |
 *       k = the nearest bin of w on the grid (grid, params: as ssq_indexed_sum; flipud: k -> rows-1-k)
 *       Tq[k] += Vq                          a cell's terms in ascending i
 *   average 0:  Cx[b,k,c] = ( sum_q hypot(Tq[k].re, Tq[k].im) ) / Q     ascending q; rounded once to `dtype`
 *   average 1:  Cx[b,k,c] = ( sum_q Tq[k] ) / Q                         ascending q; rounded once
 * Bit-reproducible from call to call; `batch` signals in one call equal `batch` calls of one signal bit for bit.
 * One kernel: a workgroup per (signal, tile of 16 or 8 columns) holds Tq in LDS; the planes are read from HBM once,
 * Cx is written once and nothing of size (Q, rows, n) is stored anywhere. Refused, with Cx unwritten: J outside
 * 1 .. 8, Q outside 1 .. 1024, rows < 2, batch or n < 1, rows > 1280 (an 8-column tile of float64 complex cells in
 * 160 KiB of LDS; 16 columns up to 640 rows), batch rows n >= 2^32, a null pointer, a proj entry that is not
 * finite, gamma < 0 or NaN. No counterpart in the reference. */
int ssq_conceft(int dtype, const void* const* V, const void* const* dV, const void* Sfs, const double* proj, void* Cx,
                int64_t batch, int64_t J, int64_t Q, int64_t rows, int64_t n, double gamma, int grid,
                const double* params, int flipud, int average, void* stream);

/* ConceFT for the CWT (ABI 112): ssq_conceft's kernel in its CWT form. The J transforms are
 * CWTs of one signal over orthogonal wavelets of equal norm (generalized Morse wavelets of orders 0 .. J-1), W_j, with
 * their time derivatives, dW_j. What differs from ssq_conceft: the phase has no Sfs term, every term carries its row's
 * weight, and all three grids are accepted (the log grids map through log2(w); w = 0 -> bin 0).
 *   W, dW   HOST arrays of J device pointers to (batch, rows, n) complex planes
 *   cst     (rows,) float64, device: the weight of row i (ssq_ssqueeze's cst with cst_f64 = 1)
 *   proj, Cx, average, flipud: as ssq_conceft; grid, params: as ssq_ssqueeze (params: 5 entries)
 * Evaluated in float64 for both dtypes (float32 planes are promoted), no contraction. Per signal b, column c,
 * projection q, with Tq a column of `rows` float64 complex cells, zero at first:
 *   for i = 0 .. rows-1 (ascending):
 *       Wq, dWq = sum_j r[q][j] * W_j[b,i,c], ... dW_j               exactly as ssq_conceft mixes V and dV
 *       if hypot(Wq.re, Wq.im) < gamma: continue
 *       w = | (dWq.im*Wq.re - dWq.re*Wq.im) / ((Wq.re^2 + Wq.im^2) * 2pi) |
 *       k = the nearest bin of w on the grid (the exact map); flipud: k -> rows-1-k
 *       Tq[k] += (Wq.re * cst[i], Wq.im * cst[i])                    a cell's terms in ascending i
 *   average 0:  Cx[b,k,c] = ( sum_q hypot(Tq[k].re, Tq[k].im) ) / Q     ascending q; rounded once to `dtype`
 *   average 1:  Cx[b,k,c] = ( sum_q Tq[k] ) / Q                         ascending q; rounded once
 * Bit-reproducible; a batch equals its single-signal calls bit for bit; the device copies of `proj` are shared with
 * ssq_conceft. Refused, with Cx unwritten, on ssq_conceft's conditions and for an unknown `grid`. No counterpart in
 * the reference. */
int ssq_conceft_cwt(int dtype, const void* const* W, const void* const* dW, const void* cst, const double* proj, void* Cx,
                    int64_t batch, int64_t J, int64_t Q, int64_t rows, int64_t n, double gamma, int grid,
                    const double* params, int flipud, int average, void* stream);

/* Time-reassigned synchrosqueezing, TSST (ABI 113; He, Cao, Zi, Zhou, Chen 2019): every
 * coefficient of an STFT moves along the time axis, within its row, to its local group delay.
 *   Sx, Vtg (batch, rows, n) complex `dtype`, device: the STFT with window g and the STFT with window tau g, tau the
 *           window's time axis in seconds, 0 at the window's centre
 *   rot     (n_fft,) complex128, device: the phase rotation table, e^{-2 pi i p / n_fft} made by the caller -- the
 *           kernel and its NumPy statement use the same bits and no sincos runs on the device. NULL: no rotation, (1, 0)
 *   Tx      (batch, rows, n) complex `dtype`; overwritten
 *   cols_per_second  fs / hop_len;  dmax: the largest displacement kept, in columns
 * Evaluated in float64 for both dtypes (float32 planes are promoted per point), basic IEEE operations only, no
 * contraction. Per signal b and row i, with Tx[b,i,:] float64 zeros at first, for c = 0 .. n-1 (ascending):
 *       gr, gi = Sx[b,i,c];  tr, ti = Vtg[b,i,c]
 *       if hypot(gr, gi) < gamma: continue              float32 planes: sqrt(gr*gr + gi*gi) in float64 (the squares
 *                                                       are exact and cannot leave the range); float64 planes: hypot
 *       s  = (tr*gr + ti*gi) / (gr*gr + gi*gi)          Re(Vtg / Sx): the group delay relative to the frame centre, s
 *       d  = rint(s * cols_per_second)                  round half to even
 *       if not (|d| <= dmax): continue                  NaN and inf included
 *       c2 = c + d;  if c2 < 0 or c2 >= n: continue
 *       p  = (i * c * hop_len) mod n_fft                exact
 *       (ur, ui) = rot ? rot[p] : (1, 0)
 *       Tx[b,i,c2] += (ur*gr - ui*gi, ur*gi + ui*gr)    a cell's terms in ascending c; re and im separate sums
 * and every cell is rounded once to `dtype`. Bit-reproducible from call to call; `batch` signals in one call equal
 * `batch` calls of one signal bit for bit. One kernel: a wavefront per (signal, row, segment of
 * ssq_time_reassign_segment() destination columns) holds its cells in LDS and walks the sources that can reach them,
 * segment + 2 dmax columns, in ascending order; no global atomics, nothing of plane size is allocated. Planes that do
 * not start on a 16-byte boundary take an element-load instance. Refused, with Tx unwritten and a message that begins
 * with the entry's name: a null Sx, Vtg or Tx; batch, rows or n < 1; batch rows n >= 2^32; n_fft < 1 (or >= 2^31) or
 * hop_len < 1; rows > n_fft; dmax < 0 or dmax > ssq_time_reassign_max_dmax() = 2^20 (a displacement and a wavefront's
 * walk stay in 32 bits); cols_per_second not finite or <= 0; gamma < 0 or NaN. No counterpart in the reference. */
int ssq_time_reassign(int dtype, const void* Sx, const void* Vtg, const void* rot, void* Tx, int64_t batch, int64_t rows,
                      int64_t n, int64_t n_fft, int64_t hop_len, double cols_per_second, int64_t dmax, double gamma,
                      void* stream);
/* The destination columns a wavefront of ssq_time_reassign owns, and the largest dmax the entry accepts. */
int ssq_time_reassign_segment(void);
int ssq_time_reassign_max_dmax(void);

/* The reassigned spectrogram (ABI 115; Kodera, Gendrin, de Villedary 1978; Auger, Flandrin 1995; DESIGN.md section
 * 4.5.9): the energy of every point of an STFT moves along both axes at once, to its instantaneous frequency (rows) and
 * its group delay (columns).
 *   Sx, dSx, Vtg (batch, rows, n) complex `dtype`, device: the STFT with window g, with its derivative g' and with
 *           tau g (tau the window's time axis in seconds, 0 at the centre). dSx may be NULL when the frequency axis is
 *           off, Vtg when dmax = 0
 *   Rx      (batch, rows, n) REAL `dtype`; overwritten
 *   acc     (batch, rows, n) uint64 and peak (batch,) uint64: caller-owned scratch, overwritten; readable afterwards
 *           (the fixed-point sums and the bits of the largest kept energy of every signal)
 *   fs, cols_per_second = fs / hop_len;  kmax, dmax: the largest displacement kept, in rows and in columns
 *   flags   SSQ_REASSIGN2D_FREQ: the frequency axis is on. dmax = 0 turns the time axis off.
 *           SSQ_REASSIGN2D_NO_WINDOW: every term goes to `acc` with a global atomic, none through the LDS window --
 *           the same bits, slower; for measurements
 * Evaluated in float64 for both dtypes (float32 planes are promoted per point), basic IEEE operations only, no
 * contraction. Per signal b, with df = fs / n_fft, for every point of row k, column c:
 *       gr, gi = Sx[b,k,c];  e = gr*gr + gi*gi
 *       kept   = not (|Sx| < gamma) and e finite        |Sx| as ssq_time_reassign takes it
 *       m  = rint(((-(di*gr - dr*gi) / e) / 6.283185307179586) / df)    dr, di = dSx[b,k,c]; rows; round half to even
 *            0 when the frequency axis is off
 *       d  = rint(((tr*gr + ti*gi) / e) * cols_per_second)              tr, ti = Vtg[b,k,c]; columns
 *            0 when dmax = 0
 *       k2 = |k + m|                                    reflected at row 0
 *       dropped: not (|m| <= kmax), k2 > rows - 1, not (|d| <= dmax), c + d outside [0, n)    (NaN included)
 *       Rx[b, k2, c + d] += e
 * The sum of a cell is taken in fixed point, so that it does not depend on the order of the additions -- on the grid, the
 * tiling or the schedule -- and is exact:
 *       emax = the largest e over the kept points of signal b (dropped ones included);  peak[b] = its bits, 0 if none
 *       ex   = frexp(emax)'s exponent:  emax = f 2^ex, 1/2 <= f < 1
 *       C    = rows * min(2 dmax + 1, n), the most terms a cell can receive;  H = bit_length(C)
 *       sh   = 62 - H - ex
 *       q    = (uint64) ldexp(e, sh), truncated: the term of a point that lands
 *       acc[b, k2, c2] = the uint64 sum of its terms, below 2^62 by construction
 *       Rx   = (dtype) ldexp((double) acc, -sh)
 * A signal without a kept point gives zeros. Every term loses less than 2^-sh to the truncation: a cell that received t
 * terms lies below the exact sum by less than t 2^-sh (2^-sh <= emax 2^(H - 61), so less than emax 2^(2H - 61) for any
 * cell), before the one rounding to `dtype` (an acc beyond 2^53 rounds once to float64 first). Bit-reproducible
 * from call to call; `batch` signals in one call equal `batch` calls of one signal bit for bit. Three launches and two
 * clears on `stream`, no host synchronisation: the peak (fetch_max on the double's bits), the scatter (a workgroup per
 * tile of ssq_reassign2d_tile(0) x ssq_reassign2d_tile(1) sources adds into an LDS window that is
 * ssq_reassign2d_tile(2) rows and ssq_reassign2d_tile(3) columns wider on every side; terms outside it are global 64-bit
 * integer atomics; at the tile's end the window's non-zero cells are added to `acc`, a wavefront per line of 64 cells, in
 * runs of neighbouring cells) and the conversion.
 * Planes that do not start on a 16-byte boundary take an element-load instance. Refused, with nothing written and a
 * message that begins with the entry's name: a null Sx, Rx, acc or peak, a null dSx with the frequency axis on, a null
 * Vtg with dmax > 0; batch, rows or n < 1; batch rows n >= 2^32; n_fft < 1 (or >= 2^31) or hop_len < 1; rows > n_fft;
 * dmax < 0 or > ssq_time_reassign_max_dmax(); kmax < 0; fs or cols_per_second not finite or <= 0; gamma < 0 or NaN;
 * rows * min(2 dmax + 1, n) >= 2^40; unknown flags. No counterpart in the reference. */
#define SSQ_REASSIGN2D_FREQ 1
#define SSQ_REASSIGN2D_NO_WINDOW 2
int ssq_reassign2d(int dtype, const void* Sx, const void* dSx, const void* Vtg, void* Rx, void* acc, void* peak,
                   int64_t batch, int64_t rows, int64_t n, int64_t n_fft, int64_t hop_len, double fs,
                   double cols_per_second, int64_t kmax, int64_t dmax, double gamma, int flags, void* stream);
/* The scatter's sizes: which = 0, 1: the rows and columns of a tile of sources; 2, 3: the rows and columns of the
 * window's halo on every side; 4: the most workgroups of the windowed scatter (with more tiles than that a workgroup
 * walks several); anything else: 0. */
int ssq_reassign2d_tile(int which);

/* The reassigned scalogram (ABI 117; Auger, Flandrin 1995): the energy of every point of a CWT
 * moves along both axes at once, to the bin of its instantaneous frequency on the synchrosqueezing grid (rows) and to its
 * group delay (columns). The CWT form of ssq_reassign2d, with which it shares the peak and conversion kernels, the shift
 * rule and the fixed-point sum.
 *   W, dW, Wd (batch, rows, n) complex `dtype`, device: the CWT over psih(w), its time derivative, and the CWT over
 *           psih'(w) (T = -1j r Wd, r = scales / fs, is the CWT taken with t psi(t)). dW may be NULL when the frequency
 *           axis is off, Wd when the time axis is
 *   cst     (rows,) float64, device: the weight of row i (ssq_ssqueeze's cst with cst_f64 = 1, da / a), >= 0 and finite
 *   rsc     (rows,) float64, device: the scale of row i in samples (columns): Re(T / W) in columns is Im(Wd / W) rsc[i]
 *   dmax    (rows,) int32, HOST: the largest displacement kept in row i, in columns; uploaded once per content
 *   home    (rows,) int32, device: the bin where the energy of row i is expected to land. It places the LDS window of a
 *           tile and changes nothing else: any values, out of range included, give the same bits
 *   Rx      (batch, rows, n) REAL `dtype`; overwritten
 *   acc     (batch, rows, n) uint64 and peak (batch,) uint64: caller-owned scratch, overwritten; readable afterwards
 *   grid, params, flipud: as ssq_ssqueeze (params: 5 entries); not looked at when the frequency axis is off
 *   flags   SSQ_REASSIGN_CWT_FREQ, SSQ_REASSIGN_CWT_TIME: the axis is on. SSQ_REASSIGN_CWT_NO_WINDOW: every term goes to
 *           `acc` with a global atomic, none through the LDS window -- the same bits; for measurements
 * Evaluated in float64 for both dtypes (float32 planes are promoted per point), basic IEEE operations only, no
 * contraction. Per signal b, for every point of row i, column c:
 *       gr, gi = W[b,i,c];  e = gr*gr + gi*gi
 *       kept   = not (|W| < gamma) and e finite          |W| as ssq_time_reassign takes it
 *       freq on:   w = | (di*gr - dr*gi) / (e * 6.283185307179586) |       dr, di = dW[b,i,c]
 *                  k = the nearest bin of w on the grid (the exact map, clamped to 0 and rows - 1 as ssq_indexed_sum
 *                      clamps it; w = 0 -> bin 0);  flipud: k -> rows-1-k
 *       freq off:  k = i
 *       time on:   d = rint(((ti*gr - tr*gi) / e) * rsc[i])                tr, ti = Wd[b,i,c]; round half to even
 *                  dropped: not (|d| <= dmax[i]) (NaN included)
 *       time off:  d = 0
 *       dropped: c + d outside [0, n)
 *       Rx[b, k, c + d] += e * cst[i]
 * The sum of a cell is ssq_reassign2d's fixed-point sum:
 *       emax = the largest e * cst[i] over the kept points of signal b (dropped ones included); peak[b] = its bits, 0 if none
 *       C    = sum_i min(2 dmax[i] + 1, n) with the frequency axis on (a bin can take points of every row),
 *              max_i min(2 dmax[i] + 1, n) with it off; dmax[i] counts as 0 with the time axis off
 *       H = bit_length(C);  sh = 62 - H - frexp(emax)'s exponent
 *       q    = (uint64) ldexp(e * cst[i], sh), truncated;  acc[b,k,c+d] = the uint64 sum of its terms, below 2^62
 *       Rx   = (dtype) ldexp((double) acc, -sh)
 * so a cell that received t terms lies below the exact sum by less than t 2^-sh, before the one rounding to `dtype`.
 * Bit-reproducible from call to call and for every `home`; `batch` signals in one call equal `batch` calls of one signal
 * bit for bit. Three launches and two clears on `stream`, no host synchronisation once the dmax table is on the device:
 * the peak, the scatter (a workgroup per tile of ssq_reassign_cwt_tile(0) x ssq_reassign_cwt_tile(1) sources adds into an
 * LDS window of ssq_reassign_cwt_tile(5) bins x ssq_reassign_cwt_tile(6) columns that starts ssq_reassign_cwt_tile(2) bins
 * below the smallest home of the tile's rows and ssq_reassign_cwt_tile(3) columns left of the tile; terms outside it are
 * global 64-bit integer atomics) and the conversion. Planes that do not start on a 16-byte boundary take an element-load
 * instance. Refused, with nothing written and a message that begins with the entry's name: a null W, cst, Rx, acc or peak,
 * a null dW or params with the frequency axis on, a null Wd, rsc or dmax with the time axis on, a null home with the
 * window on; batch or n < 1, rows < 2; batch rows n >= 2^32; gamma < 0 or NaN; an unknown grid (frequency axis on);
 * unknown flags; a dmax[i] < 0 or > ssq_time_reassign_max_dmax(); C >= 2^40. No counterpart in the reference. */
#define SSQ_REASSIGN_CWT_FREQ 1
#define SSQ_REASSIGN_CWT_TIME 2
#define SSQ_REASSIGN_CWT_NO_WINDOW 4
int ssq_reassign_cwt(int dtype, const void* W, const void* dW, const void* Wd, const double* cst, const double* rsc,
                     const int32_t* dmax, const int32_t* home, void* Rx, void* acc, void* peak, int64_t batch,
                     int64_t rows, int64_t n, double gamma, int grid, const double* params, int flipud, int flags,
                     void* stream);
/* The scatter's sizes: which = 0, 1: the rows and columns of a tile of sources; 2, 3: the window's halo in bins (below the
 * smallest home and above it + the tile's rows) and in columns (on either side); 4: the most workgroups of the windowed
 * scatter; 5, 6: the window's bins and columns; anything else: 0. */
int ssq_reassign_cwt_tile(int which);

/* The time-reassigned synchrosqueezed CWT (ABI 120): the CWT counterpart of ssq_time_reassign.
 * Every coefficient of a CWT moves along its row to its group delay, rotated to the signal's origin first, and the complex
 * terms that meet in a cell are added in signed fixed point: ssq_reassign_cwt's accumulator, re and im summed separately.
 *   W, Wd   (batch, rows, n) complex `dtype`, device: the CWT over psih(w) and the CWT over psih'(w)
 *   rsc     (rows,) float64, device: the scale of row i in samples (columns)
 *   dmax    (rows,) int32, HOST: the largest displacement kept in row i, in columns; uploaded once per content
 *   rot_lo  (rows, P) and rot_hi (rows, ceil(n / P)) complex128, device, P = SSQ_TSSQ_CWT_ROT_P: the two-level table of
 *           the rotation of row i, rot(i, c) = rot_hi[i, c / P] * rot_lo[i, c mod P] = e^{-2 pi i phi_i c}, phi_i the
 *           row's centre frequency in cycles per column: rot_lo[i, p] = exp(-2 pi i frac(phi_i p)), rot_hi[i, q] =
 *           exp(-2 pi i frac(phi_i P q)), the fractional parts exact. Both NULL: no rotation
 *   Tx      (batch, rows, n) complex `dtype`; overwritten
 *   acc     (batch, rows, n, 2) int64 and peak (batch,) uint64: caller-owned scratch, overwritten; readable afterwards
 *   flags   SSQ_TSSQ_CWT_NO_WINDOW: every term goes to `acc` with global atomics, none through the LDS window -- the same
 *           bits; for measurements
 * Evaluated in float64 for both dtypes (float32 planes are promoted per point), basic IEEE operations only, no
 * contraction. Per signal b, for every point of row i, column c:
 *       gr, gi = W[b,i,c];  e = gr*gr + gi*gi
 *       kept   = not (|W| < gamma) and e finite          |W| as ssq_time_reassign takes it
 *       d      = rint(((ti*gr - tr*gi) / e) * rsc[i])    tr, ti = Wd[b,i,c]; round half to even: ssq_reassign_cwt's d
 *       dropped: not (|d| <= dmax[i]) (NaN included);  c + d outside [0, n)
 *       (ur,ui) = (hr*lr - hi*li, hr*li + hi*lr)         (hr,hi) = rot_hi[i, c / P], (lr,li) = rot_lo[i, c mod P];
 *                                                        (1, 0) when the tables are NULL
 *       (zr,zi) = (ur*gr - ui*gi, ur*gi + ui*gr)
 *       Tx[b, i, c + d] += (zr, zi)                      a point stays in its row
 * The sum of a cell is a signed fixed-point sum, re and im separately:
 *       emax = the largest e over the kept points of signal b (dropped ones included);  peak[b] = its bits, 0 if none
 *       ex   = frexp(emax)'s exponent;  hx = ceil(ex / 2):  |zr|, |zi| <= |u| sqrt(emax) < 2^hx (1 + a few ulp)
 *       C    = max_i min(2 dmax[i] + 1, n), the most terms a cell can receive;  H = bit_length(C)
 *       sh   = 61 - H - hx
 *       q    = (int64) ldexp(z, sh), truncated toward zero, per component; a zero component adds nothing
 *       acc[b,i,c2,0..1] = the int64 sums;  |sum| <= C 2^(61 - H) (1 + a few ulp) < 2^61 (1 + a few ulp) < 2^62
 *       Tx   = (dtype) ldexp((double) acc, -sh), per component
 * The spare bit (61, not 62) pays for |u| not being exactly 1 and for an odd ex. A cell that received t terms is within
 * t 2^-sh of the exact sum in each component, before the one rounding to `dtype`; 2^-sh <= sqrt(emax) 2^(H - 60). A
 * signal without a kept point gives zeros. Bit-reproducible, independent of grid, tiling and schedule; `batch` signals in
 * one call equal `batch` calls of one signal bit for bit. Three launches and two clears on `stream`, no host
 * synchronisation once the dmax table is on the device: the peak (ssq_reassign2d's), the scatter (a workgroup per tile of
 * ssq_time_reassign_cwt_tile(0) x ssq_time_reassign_cwt_tile(1) sources, tiles starting at multiples of P, adds into an
 * LDS window of the tile's rows x ssq_time_reassign_cwt_tile(3) columns that starts ssq_time_reassign_cwt_tile(2) columns
 * left of the tile; a term outside it is two global 64-bit integer atomics) and the conversion. Planes that do not start
 * on a 16-byte boundary take an element-load instance. Refused, with nothing written and a message that begins with the
 * entry's name: a null W, Wd, rsc, dmax, Tx, acc or peak; exactly one of rot_lo and rot_hi null; batch, rows or n < 1;
 * batch rows n >= 2^31 (a cell is two words of a (rows, 2 n) view indexed in 32 bits); gamma < 0 or NaN; a dmax[i] < 0 or
 * > ssq_time_reassign_max_dmax(); unknown flags. No counterpart in the reference. */
#define SSQ_TSSQ_CWT_NO_WINDOW 1
#define SSQ_TSSQ_CWT_ROT_P 256
int ssq_time_reassign_cwt(int dtype, const void* W, const void* Wd, const double* rsc, const int32_t* dmax,
                          const void* rot_lo, const void* rot_hi, void* Tx, void* acc, void* peak, int64_t batch,
                          int64_t rows, int64_t n, double gamma, int flags, void* stream);
/* The scatter's sizes: which = 0, 1: the rows and columns of a tile of sources; 2: the window's halo in columns, on either
 * side; 3: the window's columns (the tile's plus the halo twice); 4: the most workgroups of the windowed scatter; 5: P, the columns of rot_lo
 * (= SSQ_TSSQ_CWT_ROT_P = which 1); anything else: 0. */
int ssq_time_reassign_cwt_tile(int which);

/* Fused phase transform + bin search + accumulate:
 *   for every (i, j) with |Wx[i,j]| > gamma:  Tx[k(i,j), j] += Wx[i,j] * cst[i]
 * with k from `grid`/`params` (and mirrored, k -> na-1-k, if `flipud`).
 * `Sfs` NULL selects the CWT form of w, non-NULL the STFT form.
 * `cst` is a device vector of na weights: real `dtype`, or float64 when
 * `cst_f64` != 0 (complex64 data weighted by a float64 vector accumulates in
 * double, as the reference does for 'log-piecewise' scales).
 * Tx is OVERWRITTEN (zero-filled and accumulated by the kernel).
 * `kmap` (optional, int32 (batch, na, n)) receives the bin of every point, -1 where
 * the point is below threshold.
 * replaces ssqueeze_fast -> _ssq_cwt_{log,log_piecewise,lin}[_par], _ssq_stft[_par]
 * and the CUDA strings ssq_cwt_* / ssq_stft (algos.py:126-150, 859-984, 1008-1167).
 * Summation order per output cell is ascending i, as in the reference.
 */
int ssq_ssqueeze(int dtype, const void* Wx, const void* dWx, const void* Sfs,
                 void* Tx, const void* cst, int cst_f64, int64_t batch,
                 int64_t na, int64_t n, double gamma, int grid,
                 const double* params, int flipud, int32_t* kmap, void* stream);

/* Adjoint of ssq_ssqueeze with the bins held fixed (they are integers, piecewise constant in the data):
 * gWx[a,b] (+)= |Wx[a,b]| > gamma ? cst[a] * gTx[k(a,b), b] : 0,  k as ssq_ssqueeze computes it
 * (same grid/params/flipud, `Sfs` NULL = CWT form of w, non-NULL = STFT form). `accumulate` != 0
 * adds to gWx (the direct gradient w.r.t. Wx is already there), 0 overwrites. With `cst_f64` the
 * product is formed in double and rounded once. */
int ssq_ssqueeze_adjoint(int dtype, const void* Wx, const void* dWx, const void* Sfs,
                         const void* gTx, void* gWx, int accumulate, const void* cst, int cst_f64,
                         int64_t batch, int64_t na, int64_t n, double gamma, int grid,
                         const double* params, int flipud, void* stream);

/* Same accumulate, bins taken from a precomputed phase transform `w` (inf = skip).
 * replaces indexed_sum_onfly -> _indexed_sum_{log,log_piecewise,lin}[_par] and the
 * CUDA strings indexed_sum_* (algos.py:153-250, 1169-1268). */
int ssq_indexed_sum(int dtype, const void* Wx, const void* w, void* Tx,
                    const void* cst, int cst_f64, int64_t batch, int64_t na,
                    int64_t n, int grid, const double* params, int flipud,
                    void* stream);

/* Same accumulate, bins given by the caller (ABI 118): `kidx` uint16 (batch, na, n), the bin of every point AFTER any
 * flip, 0xFFFF = skip. This is the source that carries the default reassignment of every float64 ssq_cwt; na < 65535.
 * By default the sums are accumulate_f64_kernel's where its tile fits (ssq_reassign_route): a cell is the float64 sum
 * of its terms in the order the hardware served them, rounded once to `dtype`; SSQ_TILE_ORDER=ordered (environment)
 * selects the ordered kernels, ascending i in `dtype`'s arithmetic, bit for bit ssq_indexed_sum's. Tx is OVERWRITTEN.
 * THE ENTRY DOES NOT CHECK THE MAP: the kernels index their LDS tile with it, so every entry must be 0xFFFF or < na
 * (the Python wrapper, algos.indexed_sum_bins, refuses any other map before the launch). */
int ssq_indexed_sum_bins(int dtype, const void* Wx, const void* kidx, void* Tx,
                         const void* cst, int cst_f64, int64_t batch, int64_t na,
                         int64_t n, void* stream);

/* Which kernel and build the three entries above (and every plan that reassigns through them) run for a shape, without
 * a device call (ABI 118). `binsrc`: 0 bins from dWx (ssq_ssqueeze), 1 from a stored w (ssq_indexed_sum), 2 from a
 * bin map (ssq_indexed_sum_bins, the plans' kidx); `ordered`: SSQ_TILE_ORDER=ordered is in force; `want_kmap`: the
 * caller asks for the bin map back. Outputs (any may be NULL): *kernel, one of SSQ_REASSIGN_*; *cols, the tile's
 * columns (1 for the global kernel: a thread walks one column); *wavefronts per workgroup. With cell = 8 / 16 bytes
 * (complex float32 / float64) and LDS = 160 KiB:
 *   SSQ_REASSIGN_F64     binsrc 2, not ordered, no kmap, na * n < 2^31: 32 columns while na * 32 * 16 <= LDS / 2, 16 while
 *                        na * 16 * 16 <= LDS, float64 data 8 while na * 8 * 16 <= LDS (8 wavefronts); else as below
 *   SSQ_REASSIGN_TILE16  na * 16 * cell <= LDS and na * n < 2^31: float32 32 columns while na * 32 * cell <= LDS / 2
 *                        (4 wavefronts), else 16 (2); float64 16 columns (4 wavefronts)
 *   SSQ_REASSIGN_TILE    one wavefront: 16, 8 columns while the tile fits LDS / 2, then 16, 8, 4 while it fits LDS
 *                        (16 and the half-capacity 8 are reached with na * n >= 2^31 only)
 *   SSQ_REASSIGN_GLOBAL  no LDS tile: Tx cleared, one thread per column (256-thread workgroups)
 * Returns 0, or -1 (outputs -1, 0, 0) for an unknown dtype or binsrc, an empty shape, or a bin map with na >= 65535.
 * Tests assert on it. */
#define SSQ_REASSIGN_TILE16 0     /* accumulate_tile16_kernel: ordered, DPP-combined row-lanes              */
#define SSQ_REASSIGN_TILE   1     /* accumulate_tile_kernel: ordered, one wavefront per tile               */
#define SSQ_REASSIGN_F64    2     /* accumulate_f64_kernel: unordered float64 LDS sums from a bin map      */
#define SSQ_REASSIGN_GLOBAL 3     /* accumulate_global_kernel: ordered, in global memory                   */
int ssq_reassign_route(int dtype, int binsrc, int64_t na, int64_t n, int ordered, int want_kmap,
                       int* kernel, int* cols, int* wavefronts);

/* Multisynchrosqueezing, MSST (ABI 114; Yu, Wang, Zhao 2019): the first-order frequency map
 * applied to its own output n_iter - 1 times within a column, on real-valued frequencies, then ssq_indexed_sum's
 * accumulate from the final frequency of every point.
 *   Sx      (batch, rows, n) complex `dtype`, device
 *   w       (batch, rows, n) real `dtype`: the phase transform ssq_phase_stft or ssq_stft2_phase wrote; inf = skip
 *   Tx      (batch, rows, n) complex `dtype`; overwritten
 *   wf      optional (NULL), (batch, rows, n) real `dtype`: the final frequency of every point, inf where skipped
 *   cst, cst_f64, grid, params, flipud   exactly ssq_indexed_sum's: the weights and the bins of the output
 *   f0, df  the rows' grid: row i sits at f0 + i df. The iteration runs on it, the final binning on `params`; the two
 *           need not coincide
 *   n_iter  1 .. 1024;  interp: 0 = the nearest row (the paper's form), 1 = linear interpolation between two rows
 * Per signal and column, for every row i ascending with w[i] finite (a NaN is skipped like an inf; ssq_indexed_sum
 * puts it in bin 0), in float64 for both dtypes (a float32 w is promoted), basic IEEE operations only, no contraction:
 *       f = w[i]
 *       repeat at most n_iter - 1 times:
 *           p = (f - f0) / df
 *           if not (p >= 0 and p <= rows - 1): break            NaN included
 *           r = rint(p)  (half to even);  g = w[r]
 *           interp = 1:  i0 = min(floor(p), rows - 2);  a = p - i0
 *                        if w[i0] and w[i0 + 1] are both finite:  g = w[i0] + a * (w[i0 + 1] - w[i0])
 *           if g is not finite: break                           a row that holds nothing points nowhere
 *           if g == f: break                                    a fixed point
 *           f = g
 *       fT = f rounded once to `dtype`;  wf[i] = fT
 *       k  = the bin of fT exactly as ssq_indexed_sum bins a stored w (flipud included)
 *       Tx[k] += Sx[i] * cst[i]                                 term, sum type and order (ascending i): ssq_indexed_sum's
 * With n_iter = 1, Tx is ssq_indexed_sum's bit for bit. Bit-reproducible from call to call; `batch` signals in one call
 * equal `batch` calls of one signal. One kernel: a tile of 16, 8 or 4 columns (the widest that fits) keeps its Tx cells
 * and its columns of w in LDS, 3 reals per row and column; the iteration is a loop of LDS gathers. Refused, with Tx and wf
 * unwritten and a message that begins with the entry's name: a null Sx, w, Tx, cst or params; batch or n < 1, or rows < 2;
 * rows > ssq_multi_squeeze_max_rows(dtype); batch rows n >= 2^32; n_iter outside 1 .. 1024; interp outside {0, 1}; df not
 * finite or <= 0, or f0 not finite; an unknown `grid`. No counterpart in the reference. */
int ssq_multi_squeeze(int dtype, const void* Sx, const void* w, void* Tx, void* wf,
                      const void* cst, int cst_f64, int64_t batch, int64_t rows, int64_t n,
                      double f0, double df, int64_t n_iter, int interp,
                      int grid, const double* params, int flipud, void* stream);
/* The most rows ssq_multi_squeeze takes: what a 4-column tile holds in 160 KiB of LDS, 160 KiB / (4 * 3 * sizeof real) =
 * 3413 (float32) or 1706 (float64); 0 for an unknown dtype. */
int ssq_multi_squeeze_max_rows(int dtype);

/* Multisynchrosqueezing on a table of rows (ABI 119): ssq_multi_squeeze for planes whose rows
 * are not evenly spaced -- the CWT, whose row i sits at wc fs / (2 pi scales[i]): descending, geometric on 'log' scales,
 * two geometric pieces on 'log-piecewise', hyperbolic on linear scales.
 *   Wx, w, Tx, wf, cst, cst_f64, batch, rows, n, n_iter, interp, grid, params, flipud, stream   ssq_multi_squeeze's
 *           (w: the phase transform ssq_phase_cwt or ssq_cwt2_phase wrote)
 *   fr      HOST array of `rows` float64: the rows' centre frequencies, finite and strictly monotone in either
 *           direction. Uploaded once per (device, contents) and kept; a call that finds its table enqueues no copy.
 *           The iteration runs on it, the final binning on `params`; the two need not coincide
 * Per signal and column, for every row i ascending with w[i] finite, in float64 for both dtypes (a float32 w is
 * promoted), basic IEEE operations only, no contraction; lo, hi the smaller and larger of fr[0], fr[rows - 1]:
 *       f = w[i]
 *       repeat at most n_iter - 1 times:
 *           if not (f >= lo and f <= hi): break                 NaN included
 *           i0 = the largest i <= rows - 2 with fr[i] >= f      (descending table; fr[i] <= f for an ascending one)
 *           a  = (f - fr[i0]) / (fr[i0 + 1] - fr[i0])           in [0, 1]
 *           r  = i0 + 1 if a > 0.5 or (a == 0.5 and i0 is odd), else i0        half to the even row
 *           g  = w[r]
 *           interp = 1:  if w[i0] and w[i0 + 1] are both finite:  g = w[i0] + a * (w[i0 + 1] - w[i0])
 *           if g is not finite: break
 *           if g == f: break
 *           f = g
 *       fT = f rounded once to `dtype`;  wf[i] = fT  (inf where w[i] was not finite)
 *       k  = the bin of fT exactly as ssq_indexed_sum bins a stored w (flipud included)
 *       Tx[k] += Wx[i] * cst[i]                                 term, sum type and order (ascending i): ssq_indexed_sum's
 * i0 is defined by comparisons against the table alone: the kernel finds it by a branch-free binary search of
 * ceil(log2(rows - 1)) reads, or, on a table that is geometric in one or two pieces, from a closed-form guess that it
 * checks against the table and abandons for the search when it is off by more than a row; however it is found, the bits
 * are the same. With n_iter = 1, Tx is ssq_indexed_sum's bit
 * for bit. Bit-reproducible from call to call; `batch` signals in one call equal `batch` calls of one signal. The
 * kernel is ssq_multi_squeeze's with another position rule: the table sits in LDS once per workgroup as float64, so a
 * row costs cols * 3 * sizeof(real) + 8 bytes. Refused, with Tx and wf unwritten and a message that begins with the
 * entry's name: a null Wx, w, Tx, cst, fr or params; batch or n < 1, or rows < 2; rows >
 * ssq_multi_squeeze_cwt_max_rows(dtype); batch rows n >= 2^32; n_iter outside 1 .. 1024; interp outside {0, 1}; an fr
 * entry that is not finite, or a table that is not strictly monotone; an unknown `grid`. No counterpart in the
 * reference. */
int ssq_multi_squeeze_cwt(int dtype, const void* Wx, const void* w, void* Tx, void* wf,
                          const void* cst, int cst_f64, const double* fr,
                          int64_t batch, int64_t rows, int64_t n, int64_t n_iter, int interp,
                          int grid, const double* params, int flipud, void* stream);
/* The most rows ssq_multi_squeeze_cwt takes: what a 4-column tile holds next to the table, 160 KiB / (4 * 3 * sizeof
 * real + 8) = 2925 (float32) or 1575 (float64); 0 for an unknown dtype. */
int ssq_multi_squeeze_cwt_max_rows(int dtype);
/* The columns of the tile the launcher takes for `rows` rows, the widest that fits: 16 up to 819 (float32) / 417
 * (float64) rows, 8 up to 1575 / 819, 4 up to the most rows; 0 = refused (rows < 2, too many rows, an unknown dtype).
 * No device needed. */
int ssq_multi_squeeze_cwt_tile(int dtype, int64_t rows);

/* w[q] = replacement where |ref[q]| < value.
 * replaces replace_under_abs (algos.py:498-579). */
int ssq_replace_under_abs(int dtype, void* w, const void* ref, int64_t count,
                          double value, double replacement, void* stream);

/* STFT framing: out (batch, seg_len, n_segs) <- x (batch, n_x);
 * n_segs = (n_x - seg_len) / (seg_len - n_overlap) + 1; `modulated` rotates every
 * frame by ceil(seg_len/2). replaces buffer / _buffer_gpu
 * (utils/stft_utils.py:20-138). */
int ssq_buffer(int dtype, const void* x, void* out, int64_t batch, int64_t n_x,
               int64_t seg_len, int64_t n_overlap, int modulated, void* stream);

/* Signal extension: out (batch, n1 + n + n2) <- x (batch, n).
 * replaces padsignal (utils/common.py:54-158). */
int ssq_pad_signal(int dtype, const void* x, void* out, int64_t batch, int64_t n,
                   int64_t n1, int64_t n2, int padtype, void* stream);

/* ------------------------------------------------------------------ inverses
 * Column reductions of arrays that already live on the device; sums run in the
 * reference's order (ascending row, the array's precision), results are bit-identical
 * to the NumPy expressions they replace.
 *
 * out (batch, n) <- sum_i Re(Z[b, i, :]) [/ divisor[i]].   replaces
 *   `(Wx.real / norm(scales)).sum(axis=-2)` of _icwt_1int (_cwt.py:472-476) and
 *   `Tx.real.sum(axis=0)` of issq_cwt / issq_stft (_ssq_cwt.py:369-371, _ssq_stft.py:191).
 * `divisor`: real (na,) in the data dtype, or NULL. */
int ssq_colsum(int dtype, const void* Z, const void* divisor, void* out, int64_t batch,
               int64_t na, int64_t n, void* stream);

/* Component inversion around curves: out (ncomp + 1, n) float64; row k < ncomp sums
 * Re(Z[lo[k][j] .. hi[k][j], j]) in double, row ncomp sums the rows no band covers in
 * the data dtype. lo/hi: int32 (ncomp, n), inclusive, empty when lo > hi.
 * replaces _invert_components (_ssq_cwt.py:381-403). */
int ssq_band_colsum(int dtype, const void* Z, const int32_t* lo, const int32_t* hi,
                    int64_t ncomp, double* out, int64_t na, int64_t n, void* stream);

/* ssq_band_colsum for `batch` signals: Z (batch, na, n), out (batch, ncomp + 1, n). lo/hi are (ncomp, n), shared by
 * the signals (`bands_per_signal` == 0), or (batch, ncomp, n). Each signal's result has the bits of a single call. */
int ssq_band_colsum_batch(int dtype, const void* Z, const int32_t* lo, const int32_t* hi,
                          int bands_per_signal, int64_t ncomp, double* out, int64_t batch,
                          int64_t na, int64_t n, void* stream);

/* Adjoint of ssq_colsum (the gradient of a real loss w.r.t. the complex Z, gZ = dL/dRe + i dL/dIm):
 *   gZ[b, i, j] = g[b, j] [/ divisor[i]] + 0i
 * g (batch, n) real, gZ (batch, na, n) complex, overwritten; the imaginary parts are exact zeros. One streaming pass,
 * every element written once. */
int ssq_colsum_adjoint(int dtype, const void* g, const void* divisor, void* gZ, int64_t batch,
                       int64_t na, int64_t n, void* stream);

/* Adjoint of ssq_band_colsum_batch: g (batch, ncomp + 1, n) float64 -> gZ (batch, na, n) complex of `dtype`,
 *   gZ[b, i, j] = sum over k < ncomp, ascending, of g[b, k, j] where lo[k, j] <= i <= hi[k, j]
 *               (g[b, ncomp, j] where no band holds row i) + 0i,
 * summed in float64 and rounded once. lo/hi as in ssq_band_colsum_batch. */
int ssq_band_colsum_adjoint(int dtype, const double* g, const int32_t* lo, const int32_t* hi,
                            int bands_per_signal, int64_t ncomp, void* gZ, int64_t batch,
                            int64_t na, int64_t n, void* stream);

/* Double-integral inverse CWT core: out (n_up) real <- Re ifft( sum_a fft(Wp[a]) * psih[a] ).
 * `Wp` (na, n_up) complex: the padded transform, overwritten (used as FFT workspace);
 * `psih` (na, n_up) real: wavelet samples already divided by the scale normalisation.
 * replaces the loop of _icwt_2int (_cwt.py:448-469; its (-1)^k factor and ifftshift cancel
 * for the even padded lengths it uses, and the sum over scales commutes with the iFFT). */
int ssq_icwt2(int dtype, void* Wp, const void* psih, void* out, int64_t na, int64_t n_up,
              void* stream);

/* Frequency-domain differentiation of the rows of a CWT-like array (trigdiff,
 * utils/common.py:161-245): out (rows, N) complex <- ifft(fft(Ap) * 1j * xi * fs)[:, n1 : n1 + N].
 * `Ap` (rows, n_up) complex: the (padded) rows, overwritten (FFT workspace); `xi` (n_up) real:
 * the frequency grid `_xifn(1, n_up)` in the data dtype. */
int ssq_trigdiff(int dtype, void* Ap, const void* xi, double fs, void* out, int64_t rows,
                 int64_t n_up, int64_t n1, int64_t N, void* stream);

/* Inverse STFT: x (N) <- Sx (n_fft/2 + 1, n_hops) complex. irfft of every column
 * (rocFFT), fftshift of the frame if `modulated`, overlap-add with win_a = window^a,
 * division by the overlap-added win_a1 = window^(a+1), trim of n_fft/2 leading samples.
 * replaces the body of istft (_stft.py:238-256: irfft, unbuffer, window_norm). */
int ssq_istft(int dtype, const void* Sx, const void* win_a, const void* win_a1, void* x,
              int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N, int modulated,
              void* stream);

/* ssq_istft for `batch` signals: Sx (batch, n_fft/2 + 1, n_hops), x (batch, N); a single signal is batch 1.
 *   x[b, s] = ( sum_t win_a[r] * irfft(Sx[b, :, t])[r'] ) / wn[p],   p = s + n_fft/2, r = p - t hop_len in [0, n_fft),
 *   r' = r rotated by n_fft/2 if `modulated`, wn[p] = sum_t win_a1[p - t hop_len] over t < (N - 1) / hop_len + 1
 *   (no division where wn <= the dtype's smallest normal number).
 * The route is the one ssq_istft_algo names: "fused" -- one LDS-transform kernel for the whole batch that overlap-adds
 * the frames of an item in LDS (no frame reaches memory), then a pass that adds neighbouring strips in ascending order,
 * divides by wn (computed once per call) and trims -- or "rocfft": ssq_istft's route, a signal at a time. Each
 * signal's result does not depend on the batch it is in. */
int ssq_istft_batch(int dtype, const void* Sx, const void* win_a, const void* win_a1, void* x,
                    int64_t batch, int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N,
                    int modulated, void* stream);

/* Adjoint of ssq_istft_batch (gSx = dL/dRe(Sx) + i dL/dIm(Sx) of a real loss with gradient g w.r.t. x):
 * g (batch, N) real -> gSx (batch, n_fft/2 + 1, n_hops) complex, overwritten.
 *   u[p] = g[p - n_fft/2] / wn[p]  (g[...] itself where the forward did not divide; 0 outside the N samples)
 *   gSx[k, t] = (c_k / n_fft) * rfft_k( win_a[r] * u[t hop_len + r] ),  the frame rotated as in the forward,
 *   c_k = 1 for DC and (even n_fft) Nyquist, 2 elsewhere; the imaginary parts of those bins are exact zeros.
 * "fused" shapes run the forward STFT's LDS-transform kernel on u (zero-extended on the fly) with the weights applied
 * where a bin is stored; the others frame u, window it, run rocFFT's real forward transform and weight the result.
 * Two calls on the same input give the same bits. */
int ssq_istft_adjoint(int dtype, const void* g, const void* win_a, const void* win_a1, void* gSx,
                      int64_t batch, int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N,
                      int modulated, void* stream);

/* The route ssq_istft_batch / ssq_istft_adjoint take for a shape: "fused" (float32, n_fft a power of two in
 * [128, 2048], n_hops == (N - 1) / hop_len + 1) or "rocfft" (everything else). */
const char* ssq_istft_algo(int dtype, int64_t n_fft, int64_t n_hops, int64_t hop_len, int64_t N);

/* ------------------------------------------------------------ ridge extraction
 * The loop nests of extract_ridges (ridge_extraction.py:113-232) on arrays that are
 * already on the device; (na, n) arrays are row-major, real, in `dtype`.
 *
 * energy <- |Tf|^2, `np.abs(Tf)**2` (:129). Tf: (na, n) complex (interleaved) when
 * `is_complex`, else real. */
int ssq_ridge_energy(int dtype, int is_complex, const void* Tf, void* energy, int64_t na,
                     int64_t n, void* stream);

/* E <- -log(energy / max_i energy[i, j] + eps)   (:138-139). */
int ssq_ridge_neglog(int dtype, const void* energy, void* E, double eps, int64_t na, int64_t n,
                     void* stream);

/* Forward-backward tracking (fw_bw_ridge_tracking, :91-111 -> :143-232):
 *   pe[f, t] = E[f, t] + min_g(pe[g, t-1] + P[f, g]),  P[f, g] = penalty * (sc[f] - sc[g])^2
 *   ridge[t] = argmin_f pe[f, t], then for t = n-2 .. 0 the last f with
 *   |pe[r, t+1] - E[r, t+1] - (pe[f, t] + P[r, f])| < eps, r = ridge[t+1], if any.
 * `sc` (na,): the (log) scales in the penalty dtype -- float32 when `penalty_f32`
 * (every input but complex128, :113-117), else float64; `pe` (na, n) and `ridge` (n,)
 * int64 are outputs. Bit-identical to the reference's loops for identical E.
 * Rows: one workgroup walks the time axis with a column of `pe` and of `E` in its 160 KiB
 * of LDS, which holds at most 4549 rows of float32 data, 2408 rows of float64 data with
 * float32 penalties, 2274 rows of float64 data with float64 penalties. One row more is
 * refused (-1, "... rows do not fit the workgroup's LDS") before anything is launched:
 * `pe` and `ridge` keep what they held. */
int ssq_ridge_track(int dtype, int penalty_f32, const void* E, void* pe, const void* sc,
                    double penalty, double eps, int64_t na, int64_t n, int64_t* ridge,
                    void* stream);

/* ridge_e[j] <- energy[ridge[j], j] (NULL: skipped), then
 * energy[int(ridge[j] - bw) : int(ridge[j] + bw), j] = 0 with Python's slice rules (:142-150). */
int ssq_ridge_clear(int dtype, void* energy, const int64_t* ridge, double bw, void* ridge_e,
                    int64_t na, int64_t n, void* stream);

/* The three steps above over `batch` transforms at once (ABI 103): contiguous (batch, na, n) arrays, `ridge`
 * and `ridge_e` (batch, n); one workgroup per transform in the tracking passes -- a pass is one workgroup's
 * walk over time, so a batch costs about what one transform does until the CUs run out. No counterpart in the
 * reference (its extract_ridges takes one transform); results per transform are those of the calls above. */
int ssq_ridge_neglog_batch(int dtype, const void* energy, void* E, double eps, int64_t na, int64_t n,
                           int64_t batch, void* stream);
int ssq_ridge_track_batch(int dtype, int penalty_f32, const void* E, void* pe, const void* sc,
                          double penalty, double eps, int64_t na, int64_t n, int64_t* ridge,
                          int64_t batch, void* stream);
int ssq_ridge_clear_batch(int dtype, void* energy, const int64_t* ridge, double bw, void* ridge_e,
                          int64_t na, int64_t n, int64_t batch, void* stream);

/* ----------------------------------------------------------------- CWT plan
 * Replaces the body of cwt() (_cwt.py:255-306: pad -> fft -> Psih*xh -> ifft
 * [-> *1j*xi/dt -> ifft] -> unpad) and, when ssq parameters are set, the
 * ssq_cwt() tail (_ssq_cwt.py:266-289 -> ssqueezing.py:122-146).
 *
 * The filter bank is passed in *banded* form: row i is non-negligible only on DFT
 * bins [band_lo[i], band_lo[i] + band_len[i]) of the M-point grid (bins above M/2
 * are negative frequencies); its values are bank[band_off[i] .. band_off[i+1]).
 * The Nyquist bin must already be halved (wavelets.py:86-95).
 */
typedef struct ssq_cwt_plan ssq_cwt_plan;

typedef struct {
    int      dtype;        /* SSQ_F32 | SSQ_F64 (the wavelet's dtype)             */
    int      padtype;      /* SSQ_PAD_*                                           */
    int64_t  n;            /* signal length N                                     */
    int64_t  m;            /* padded length M (== n when padtype NONE)            */
    int64_t  n1;           /* left pad                                            */
    int64_t  na;           /* number of scales                                    */
    const void*    bank;       /* host, real dtype, concatenated band values     */
    const int64_t* band_off;   /* host, na + 1                                    */
    const int32_t* band_lo;    /* host, na                                        */
    double   dt;           /* sampling period (derivative multiplier 1j*xi/dt)    */
    const void*    row_scale;  /* host, na reals or NULL: per-row output scaling  */
                               /* (sqrt(scale) when l1_norm=False, _cwt.py:307)   */
    int64_t  max_batch;    /* largest batch the plan will be executed with        */
    int      algo;         /* 0 = auto, 1 = force generic (rocFFT) path           */
} ssq_cwt_desc;

int  ssq_cwt_plan_create(ssq_cwt_plan** plan, const ssq_cwt_desc* desc);
void ssq_cwt_plan_destroy(ssq_cwt_plan* plan);

/* Synchrosqueezing parameters for subsequent executes (host pointers, copied). */
int  ssq_cwt_plan_set_ssq(ssq_cwt_plan* plan, int grid, const double* params,
                          const void* cst, int cst_f64, int flipud, double gamma);

/* x: (batch, n) real `dtype` on the device. Outputs (any may be NULL):
 *   Wx, dWx, Tx : (batch, na, n) complex;   w : (batch, na, n) real.
 * `rpadded` != 0 returns Wx/dWx of padded width m instead (Tx/w must be NULL).
 * Tx requires ssq_cwt_plan_set_ssq(); bins come from dWx (fused form) unless `w` is
 * requested, in which case they come from the rounded `w` (two-step form,
 * get_w=True in the reference). */
int  ssq_cwt_execute(ssq_cwt_plan* plan, const void* x, int64_t batch, void* Wx,
                     void* dWx, void* Tx, void* w, int rpadded, void* stream);
/* Adjoint of the plan's CWT (ABI 108; the gradient of a real loss w.r.t. the real input, torch's convention
 * gx = Re(A^H g)):
 * gx (batch, n) real  <-  gWx, gdWx (batch, na, n) complex, (batch, na, m) with `rpadded` != 0; either may be NULL (not
 * both). With F_a = fft_m(U gWx_a), G_a = fft_m(U gdWx_a) -- U puts the n columns at offset n1 of a zero row of length
 * m, the identity with `rpadded` --
 *   gx = pad^T Re ifft_m( sum_a s_a psi_a[k] (F_a[k] - i m_k G_a[k]) )
 * psi_a: row a of the banded bank (zero outside its band), s_a: row_scale (1 when NULL), m_k: the forward's derivative
 * multiplier (xi_k / dt in the plan dtype), ifft_m normalised by 1 / m, pad^T: every sample receives the sum of its
 * padded copies (zero padding contributes nothing). gx is overwritten; the same input gives the same bits, alone or in
 * any batch. Rows go through the product workspace of the exact forward path in the same chunks (allocated at the
 * first call that needs it), batched rocFFT row transforms, one kernel that reads the banded bank and skips the rows
 * whose band does not reach a bin, one inverse transform per signal and an unpadding pass. batch in [1, max_batch]. */
int  ssq_cwt_adjoint(ssq_cwt_plan* plan, const void* gWx, const void* gdWx, void* gx,
                     int64_t batch, int rpadded, void* stream);

/* Optional fast path ("overlap-save zoom" iFFT, float32 or float64, power-of-two m,
 * analytic bank): tables planned on the host (ssqueezepy_amd/_blocks.py documents the
 * decomposition; all pointers are host arrays, copied). Rows with class -1 in `rows`
 * -- listed in `generic_rows` -- keep using the exact full-length path.
 * Must be called before the first execute. No reference counterpart: the reference
 * evaluates every row as one length-m inverse FFT (_cwt.py:167-177); this is the
 * same filter bank applied block-wise. */
typedef struct {
    int            n_classes;
    const int64_t* classes;      /* n_classes x 5: P, margin, valid, blocks/signal, analytic   */
                                 /* (1: blocks of the analytic signal, for rows continued past */
                                 /* the Nyquist bin; such classes come last)                   */
    const int32_t* rows;         /* na x 6: class, kappa_lo, K_P, L', G, pbank_off  */
    const void*    pbank;        /* P-grid band values of the block rows (plan dtype) */
    const void*    pxi;          /* xi at the same bins (same indexing, plan dtype)   */
    int64_t        n_pbank;
    const void*    ctw;          /* complex column twiddles exp(2i pi q/P) (plan dtype) */
    const int64_t* ctw_off;      /* n_classes + 1                                   */
    const void*    ftw;          /* complex FFT twiddles exp(2i pi q/L') (plan dtype) */
    int64_t        n_ftw;
    int64_t        ftw_off[5];   /* per L' = 128, 256, 512, 1024, 2048              */
    const int32_t* items[5];     /* per L': n_items x 4: row, block, c0, class      */
    int64_t        n_items[5];
    const int32_t* generic_rows; /* rows left on the exact path                     */
    int64_t        n_generic;
} ssq_cwt_blocks_desc;

int  ssq_cwt_plan_set_blocks(ssq_cwt_plan* plan, const ssq_cwt_blocks_desc* desc);

/* Optional column-tile path of the fused ssq_cwt form (float32, power-of-two m, block
 * tables set, Tx requested without w): rows that are at least 2x oversampled after a
 * decimation by R >= 4 are not transformed at full length at all. Their band is
 * inverse-transformed at length m / R into a plan-owned intermediate, and one kernel per
 * 64-column tile interpolates Wx / dWx from it (8-tap Kaiser-Bessel kernel and its
 * derivative, modulation by hardware sin / cos of an exact phase), writes Wx, and reassigns
 * into an LDS-resident tile of Tx in ascending row order -- Wx is never read back and no bin map is written for those rows. The other
 * rows keep the block / exact kernels; the tile kernel reads their Wx and bin map back.
 * ssqueezepy_amd/_tiles.py documents the decomposition and builds the tables (host
 * arrays, copied). Must follow ssq_cwt_plan_set_blocks, before the first execute.
 * Replaces, for those rows, _cwt.py:167-177 (ifft of Psih*xh, and of its 1j*xi multiple)
 * together with ssqueezing.py:122-146 -> algos.py:859-953 (the reassignment loop). */
typedef struct {
    int32_t        n_segs;
    const int32_t* segs;         /* n_segs x 8: kind (0 read back, 1 interpolate), first step, */
                                 /* steps, log2 R, weight-table offset (phases), intermediate  */
                                 /* stride per signal, L - 1, class offset (complex entries)   */
    int32_t        n_steps;
    const int32_t* rows;         /* 4 n_steps x 4: row (sign bit: repeats the previous row to  */
                                 /* pad a step), offset in class, kc, theta = 2 pi kc / (m dt) */
                                 /* (float bits). The rows of a step are consecutive.           */
    const void*    wtab;         /* float32 [n_phases][16]: per tap, phi and phi' / (R dt)     */
    int64_t        n_phases;
    const void*    tbank;        /* float32: band values / (phi_hat m) of the interpolated rows */
    int64_t        n_tbank;
    int32_t        n_irows;
    const int64_t* irows;        /* n_irows x 8: row, lo, K, kc, L, tbank offset, class, index in class */
    int32_t        n_classes;
    const int64_t* classes;      /* n_classes x 4: L, rows, entries per signal before it, log2 R */
    int64_t        u_total;      /* complex entries of the intermediate per signal             */
    int64_t        n_items_tile[5]; /* per L': leading block items that remain (rows read back) */
    int32_t        reserved;     /* rows per step of `rows` (0 = 4): must equal ssq_cwt_tile_rows_per_step() */
} ssq_cwt_tiles_desc;

int  ssq_cwt_plan_set_tiles(ssq_cwt_plan* plan, const ssq_cwt_tiles_desc* desc);

/* Per-stage timing with HIP events on the execute stream (measurement aid, off by
 * default; execute synchronises when it is on). `stage_ms[4]` receives the time
 * accumulated since the last reset: 0 = pad + forward FFT + block spectra, 1 = block
 * rows, 2 = exact / generic rows, 3 = reassignment; `*signals` the transforms covered.
 * `enable` = 1 / 0 switches timing on / off and resets the accumulators, -1 only reads. */
int  ssq_cwt_plan_timing(ssq_cwt_plan* plan, int enable, double* stage_ms, int64_t* signals);

/* signals a plan processes per kernel launch (its launch group; the batch is walked in
 * groups of this size) */
int  ssq_cwt_plan_group(const ssq_cwt_plan* plan);

/* What executed: the number of column tiles the column-tile kernel has finished on this plan
 * since its creation (0 without tile tables). Synchronises `stream`. An execute that took the
 * tile path adds batch * ceil(n / ssq_cwt_plan_tile_cols(plan)) (tile kernel 3 with an odd left padding: ceil((n + 1) /
 * 32) -- its tiles start one column early); one that took the block path +
 * separate reassignment adds nothing. (Tests assert on this rather than on the plan's `algo`
 * label.) */
int64_t ssq_cwt_plan_tiles_done(ssq_cwt_plan* plan, void* stream);
/* Columns per tile of the kernel the next execute launches: 32 or 16 (float64 tile in LDS,
 * unordered ds_add_f64 accumulation -- the default), 64 with SSQ_TILE_ORDER=ordered in the
 * environment (float32 tile, terms added in the reference's row order; na <= 318). 0 without
 * tile tables. */
int  ssq_cwt_plan_tile_cols(const ssq_cwt_plan* plan);
/* Which column-tile kernel the next execute launches (ABI 105): 0 none, 1 the ordered float32 tile
 * (SSQ_TILE_ORDER=ordered), 2 the float64 tile with one column per lane (tile2_kernel), 3 the float64 tile with a
 * column pair per lane (tile3_kernel: the default whenever the tile holds 32 columns, i.e. up to 318 rows;
 * SSQ_DEBUG_TILE_PAIR=0 switches it off). Same results in 2 and 3. */
int  ssq_cwt_plan_tile_kernel(const ssq_cwt_plan* plan);
/* Diagnostic (ABI 105): the first `n` (<= 512) 64-bit words of the tile path's counter block -- word 0 = tiles done (as
 * above); words 64.. = per-wavefront shader-clock sums per phase of workgroup 0, filled by profiling builds of the tile
 * kernel only (-DSSQ_T3_PROF=1, tools/r6), zero otherwise. Synchronises `stream`. */
int  ssq_cwt_plan_tile_counters(ssq_cwt_plan* plan, unsigned long long* out, int n, void* stream);

/* Diagnostic (tests; not needed by a caller of the transforms): from now on every fused execute
 * (Tx requested, bins from dWx) also writes the bin index of every point AS THE REASSIGNMENT CONSUMED
 * IT -- 0 .. na-1, 0xFFFF for a point below gamma -- to `kmap`, a caller-owned device array
 * (batch, na, n) of uint16; NULL switches it off. On the column-tile path the default tile kernel
 * (a separate diagnostic build of it: uniform reassignment weights, i.e. 'log' scales, 16 wavefronts)
 * stores the bins it computes for the rows it interpolates and the ones it reads back for the others;
 * on the block path + separate reassignment the plan's own bin map is copied. With
 * SSQ_TILE_ORDER=ordered on the tile path the execute fails (that kernel's Tx is the CPU loop's bit
 * for bit, which pins its bins). Replaces the reference's `ssqueeze_fast(..., get_k)`-style
 * introspection: /root/reference has none (algos.py:859-984 computes k inline), the oracle's
 * `get_k` is the other side of the comparison. */
int  ssq_cwt_plan_set_bin_dump(ssq_cwt_plan* plan, unsigned short* kmap);

/* Rows per step the tile kernel of this build walks (4; the host tables of
 * ssq_cwt_plan_set_tiles must be built for the same number: `rows` holds that many records per
 * step). */
int  ssq_cwt_tile_rows_per_step(void);

/* bytes of device memory held by the plan (bank + workspace) */
int64_t ssq_cwt_plan_bytes(const ssq_cwt_plan* plan);
/* name of the compute path the plan selected ("rocfft", "zoom+rocfft", ...) */
const char* ssq_cwt_plan_algo(const ssq_cwt_plan* plan);

/* ---------------------------------------------------------------- STFT plan
 * Replaces the body of stft() (_stft.py:127-147,166-170: pad -> buffer -> *window
 * -> rfft along the frame axis) and, with ssq parameters, the ssq_stft() tail
 * (_ssq_stft.py:102-122).
 */
typedef struct ssq_stft_plan ssq_stft_plan;

typedef struct {
    int      dtype;
    int      padtype;
    int64_t  n;            /* signal length                                       */
    int64_t  n_fft;        /* frame length                                        */
    int64_t  hop_len;
    int      modulated;
    const void* window;       /* host, n_fft reals (already ifftshift-ed if        */
    const void* diff_window;  /* modulated; diff_window already times fs), or NULL */
    int64_t  max_batch;
} ssq_stft_desc;

int  ssq_stft_plan_create(ssq_stft_plan** plan, const ssq_stft_desc* desc);
void ssq_stft_plan_destroy(ssq_stft_plan* plan);
int  ssq_stft_plan_set_ssq(ssq_stft_plan* plan, const void* Sfs, int grid,
                           const double* params, const void* cst, int cst_f64,
                           int flipud, double gamma);
/* rows = n_fft/2 + 1, n_hops = (n - 1) / hop_len + 1 -> query */
int  ssq_stft_plan_shape(const ssq_stft_plan* plan, int64_t* rows, int64_t* n_hops);
/* name of the route the plan takes for the framing + window + FFT stage: "fused" (float32, n_fft a power of
 * two in [128, 2048]: one launch, LDS transform), "fused-mixed-radix" (float32, any other n_fft whose prime
 * factors are <= 31 and that fits the LDS: one launch, mixed-radix LDS transform -- the reference's benchmark
 * shape n_fft = 598, examples/benchmarks.py:78-79), "rocfft" (everything else, float64: framing kernel + batched
 * rocFFT with strided output). Tests assert on it. */
const char* ssq_stft_plan_algo(const ssq_stft_plan* plan);
/* What a float32 plan of window length n_fft runs when its route is "fused-mixed-radix", without a plan and without a
 * device call (ABI 116): 1 and the passes' radices in order (radix[0 .. *npass), the rest of the 10 entries 0 -- 16s,
 * 8s, 4s, a 2, then the odd primes 3 .. 31 ascending) and the frames a workgroup transforms together (*G: 16, 8, 4, 2 or
 * 1), or 0 (outputs zeroed) where that kernel does not take n_fft: the powers of two 128 .. 2048 ("fused"), a prime
 * factor above 31, more than 10 passes, n_fft above 4992 ("rocfft"). Any of the pointers may be NULL. Tests assert
 * on it. */
int  ssq_stft_generic_shape(int64_t n_fft, int* radix /*[10]*/, int* npass, int* G);
/* x: (batch, n). Sx, dSx, Tx: (batch, rows, n_hops) complex; w: real. */
int  ssq_stft_execute(ssq_stft_plan* plan, const void* x, int64_t batch, void* Sx,
                      void* dSx, void* Tx, void* w, void* stream);
/* Adjoint of the plan's STFT (the gradient of a real loss w.r.t. the real input, torch's convention gx = Re(A^H g)):
 * gx (batch, n) real  <-  gSx, gdSx (batch, rows, n_hops) complex; either may be NULL (not both).
 * gx = pad^T ( sum_t  win[m - t*hop]  * Re F^-1(gSx[:, t])[m - t*hop]
 *            +        dwin[m - t*hop] * Re F^-1(gdSx[:, t])[m - t*hop] )
 * F^-1(g)[n] = sum_{k=0}^{n_fft/2} g[k] e^{+2 pi i k n / n_fft}: one-sided, no 1/n_fft, no doubling (the imaginary
 * parts of DC and Nyquist do not contribute). Window, diff-window, padtype, modulation, hop and n are the plan's; gx is
 * overwritten; two calls on the same input give the same bits. "fused" plans (ssq_stft_plan_algo) run one LDS-transform
 * kernel and a short unpadding pass, the others rocFFT's inverse real transform, an overlap-add and the same pass. */
int  ssq_stft_adjoint(ssq_stft_plan* plan, const void* gSx, const void* gdSx, void* gx,
                      int64_t batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSQ_HIP_H */
