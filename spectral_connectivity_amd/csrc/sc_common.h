// sc_common.h -- shared host/device helpers of libsc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/sc_hip.h"
#include "sc_complex.h"

void sc_set_error(const char* fmt, ...);
struct ScRec;         // (accumulator records and their CSM view: below)
struct ScCsmView;

// Diagnostic switches (ablation / A-B tools, tests of alternative kernels): environment variables read ONCE when the library is
// loaded and again whenever the host calls sc_debug_reload_env() -- no getenv on a launch path.  sc_switch(id) is the value
// string or nullptr when the variable is unset.
enum ScSwitch {
    SC_SW_FUSED_DEBUG, SC_SW_FUSED2_TERMS, SC_SW_FUSED_SPLIT, SC_SW_FUSED_NO_SMALL, SC_SW_MTFFT_DEBUG, SC_SW_MTFFT_WIDE,
    SC_SW_MTFFT_F64, SC_SW_F64_SPLIT, SC_SW_F64_OC, SC_SW_F64_NO_FORK, SC_SW_F64_NO_BLOCK, SC_SW_WILSON_FFT, SC_SW_GLOBAL_EIG,
    SC_SW_GLOBAL_NT256, SC_SW_GRANGER_KERNEL, SC_SW_FUSED_FOLD_OBS, SC_SW_MTFFT_LONG, SC_SW_CANON_EIG, SC_SW_MTFFT_MIXED, SC_SW_MTFFT_MIXED_GEO, SC_SW_MTFFT_SLICE, SC_SW_MVAR_INVERSE, SC_SW_FUSED_SPLIT_TAIL,
    SC_SW_SEED_JACKKNIFE_CHUNK, SC_SW_COUNT
};
const char* sc_switch(int id);

// sc_api.hip: Z[rows][F] -> X[f][b_off + row] (X has `batch` columns), imaginary part of rows 0 and nyquist_row zeroed
int sc_internal_rows_to_bins(const void* d_Z, void* d_X, int64_t rows, int64_t F, int64_t batch, int64_t b_off,
                             int64_t nyquist_row, hipStream_t st);

// sc_mtfft_long.hip: stage A for long power-of-two windows (two half-workgroups in anti-phase)
bool sc_internal_mtfft_long_applies(int64_t N, int64_t C, int64_t groups);
int64_t sc_internal_mtfft_long_coverage(int64_t N, int64_t C);
int sc_internal_mtfft_long(const float* d_x, int64_t T, int64_t R, int64_t C, int64_t L, int64_t step, int64_t W, int64_t N,
                           const float* d_tapers, int64_t K, int detrend_type, const void* d_twiddles, void* d_X, void* d_P,
                           const float* d_scale, hipStream_t st);

// sc_mtfft_mixed.hip: stage A for the window lengths N = 10 RM RF that are not powers of two (register-resident radix-10 passes,
// anti-phase half-workgroups, planes-format output)
bool sc_internal_mtfft_mix_has(int64_t N);
bool sc_internal_mtfft_mix_applies(int64_t N, int64_t C, int64_t groups);
int64_t sc_internal_mtfft_mix_coverage(int64_t N, int64_t C, bool planes);
int sc_internal_mtfft_mix(const float* d_x, int64_t T, int64_t R, int64_t C, int64_t L, int64_t step, int64_t W, int64_t N,
                          const float* d_tapers, int64_t K, int detrend_type, const void* d_twiddles, void* d_X, void* d_P,
                          const float* d_scale, hipStream_t st);

// sc_api.hip: process-wide cache of the batched in-place complex128 rocFFT plans of the Wilson kernels (never destroyed: see there);
// *cached == false: the table is full and the caller destroys the plan
struct rocfft_plan_t;
int sc_internal_z2z_plan(struct rocfft_plan_t** plan, int forward, size_t N, size_t batch, bool* cached);

// sc_wilson_fft.hip: A <- fft(causal(ifft(A))) in one kernel, for the lengths `supported` accepts
bool sc_internal_causal_fft_supported(int64_t N);
bool sc_internal_causal_fft_natural_supported(int64_t N);
int sc_internal_causal_fft_pair_natural(void* d_A, const int32_t* d_status, int64_t n_problems, int C, int64_t N,
                                        hipStream_t st);
int sc_internal_causal_fft_pair(void* d_A, const int32_t* d_status, int64_t n_problems, int C, int64_t N,
                                hipStream_t st);

// sc_wilson_pair.hip: pairwise Granger with the 2 x 2 Wilson iteration of a pair resident on one compute unit
bool sc_internal_granger_resident_applies(int64_t n_freq_accum, int64_t N);
int sc_internal_granger_resident(const void* d_accum, int64_t n_groups, const ScCsmView& v, int64_t C, uint32_t planes,
                                 const int32_t* d_pairs, int64_t n_pairs, double tol, int max_iter, void* d_work, size_t work_bytes,
                                 int keep_output, double* d_out, int32_t* d_n_iter, int32_t* d_status, int32_t* h_summary,
                                 hipStream_t st);

// sc_memory.hip: d_out[0 .. n) = NaN (the default of every stage-D output that is not KEEP_OUTPUT)
void sc_internal_fill_nan(double* d_out, int64_t n, hipStream_t st);

// sc_wilson.hip: the epilogue of pairwise Granger on factors G [P][4][g_stride] (lam, Hinv, rot per pair from d_h0 [P][4], then the
// prediction on the bins f <= N/2 into d_out); queued on st, not synchronised.  d_hinv, d_rot: [P][4] scratch.
void sc_internal_granger_epilogue(const void* d_G, int64_t g_stride, const double* d_h0, double* d_hinv, double* d_rot,
                                  ScRec accum, const ScCsmView& v, const int32_t* d_pairs, int64_t n_groups,
                                  int64_t n_pairs, int64_t C, double* d_out, hipStream_t st);

// sc_mvar.hip: the explicit inverse and the matrix-core product of the full Wilson factorisation on caller buffers
// (natural-layout C x C complex128 matrices; see there)
int sc_internal_mvar_inverse(int64_t C, int64_t P, int64_t N, int64_t n_bins, const void* d_M, void* d_out, void* scratch,
                             const double* d_zero, hipStream_t st);
int sc_internal_mvar_gemm(int64_t C, int64_t n_problems, int64_t n_bins, const void* X, int64_t x_sp, int64_t x_sn,
                          const void* Y, int64_t y_sp, int64_t y_sn, void* O, int64_t o_sp, int64_t o_sn, hipStream_t st);

// sc_timing.hip: brackets the launches of an entry point with two hipEvents on its stream while sc_timing_enable(1)
struct ScTimed {
    int slot;
    void* st;
    ScTimed(const char* name, void* stream);
    ~ScTimed();
    ScTimed(const ScTimed&) = delete;
    ScTimed& operator=(const ScTimed&) = delete;
};

#define SC_CHECK_HIP(expr)                                                        \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            sc_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                         __FILE__, __LINE__);                                     \
            return SC_EHIP;                                                       \
        }                                                                         \
    } while (0)

#define SC_REQUIRE(cond, msg)                                                     \
    do {                                                                          \
        if (!(cond)) {                                                            \
            sc_set_error("invalid argument: %s (%s)", msg, #cond);                \
            return SC_EINVAL;                                                     \
        }                                                                         \
    } while (0)

// The tail of an entry point: waits for the stream; a failed wait or launch before it is reported as "<what> failed: <error>".
inline int sc_sync_or_report(hipStream_t st, const char* what) {
    if (hipStreamSynchronize(st) == hipSuccess && hipGetLastError() == hipSuccess) return SC_OK;
    sc_set_error("%s failed: %s", what, hipGetErrorString(hipGetLastError()));
    return SC_EHIP;
}

// Accumulator records as their consumers see them: float elements (f32 engine) or double elements (f64 engine,
// SC_RECORD_F64 set in `planes`).  Pointer arithmetic in elements, loads widened to double.
struct ScRec {
    const void* p;
    int f64;
    __host__ __device__ ScRec operator+(int64_t n) const { return ScRec{(const char*)p + n * (f64 ? 8 : 4), f64}; }
    __device__ double operator[](int64_t i) const {
        return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
    }
};
__host__ inline ScRec sc_rec(const void* d_accum, uint32_t planes) { return ScRec{d_accum, (planes & SC_RECORD_F64) ? 1 : 0}; }

#define SC_TILE 16            // channel tile edge of the accumulator layout
#define SC_TILE_ELEMS 256
#define SC_MAX_SIGNALS 256    // v1 kernels stage all channels of an observation row in LDS

// number of planes / offset (in planes) of a plane inside a bin record
__host__ __device__ inline int sc_plane_count(uint32_t planes) {
    int n = 0;
    if (planes & SC_PLANE_CSM) n += 2;
    if (planes & SC_PLANE_ABS_IM) n += 1;
    if (planes & SC_PLANE_IM_SQ) n += 1;
    if (planes & SC_PLANE_SIGN_IM) n += 1;
    if (planes & SC_PLANE_UNIT) n += 2;
    return n;
}
__host__ __device__ inline int sc_plane_offset(uint32_t planes, uint32_t which) {
    int n = 0;
    if (which == SC_PLANE_CSM) return n;
    if (planes & SC_PLANE_CSM) n += 2;
    if (which == SC_PLANE_ABS_IM) return n;
    if (planes & SC_PLANE_ABS_IM) n += 1;
    if (which == SC_PLANE_IM_SQ) return n;
    if (planes & SC_PLANE_IM_SQ) n += 1;
    if (which == SC_PLANE_SIGN_IM) return n;
    if (planes & SC_PLANE_SIGN_IM) n += 1;
    return n;  // SC_PLANE_UNIT
}
__host__ __device__ inline int sc_n_blocks(int64_t C) { return (int)((C + SC_TILE - 1) / SC_TILE); }
__host__ __device__ inline int sc_n_tiles(int nb) { return nb * (nb + 1) / 2; }
// packed index of upper tile (bi <= bj)
__host__ __device__ inline int sc_tile_index(int bi, int bj, int nb) {
    return bi * nb - bi * (bi - 1) / 2 + (bj - bi);
}

// CSM records as every stage-D consumer reads them: F = N or N/2+1 bins per group (N/2+1: real input, S(-f) = conj S(f)
// completes the bins past N/2), upper-triangular 16 x 16 tiles of un-normalised sums divided by n_obs.  sc_csm_view: from the
// arguments of an entry point (d_accum non-NULL); consumers of single bins (sc_canonical.hip) pass N = F = their bin count.
struct ScCsmView {
    int64_t N, F, floats_per_bin;
    int NB, n_tiles, p_csm, two_sided;
    double n_obs;
};
inline int sc_csm_view(uint32_t planes, int64_t n_freq_accum, int64_t N, int64_t C, int64_t n_obs, ScCsmView* v) {
    SC_REQUIRE(planes & SC_PLANE_CSM, "accumulator record must contain SC_PLANE_CSM");
    SC_REQUIRE(n_freq_accum == N || n_freq_accum == N / 2 + 1, "accumulators must hold N or N/2+1 bins");
    SC_REQUIRE(n_obs >= 1, "n_observations must be positive");
    v->N = N; v->F = n_freq_accum;
    v->NB = sc_n_blocks(C); v->n_tiles = sc_n_tiles(v->NB);
    v->p_csm = sc_plane_offset(planes, SC_PLANE_CSM);
    v->two_sided = n_freq_accum == N ? 1 : 0;
    v->floats_per_bin = (int64_t)sc_plane_count(planes) * v->n_tiles * SC_TILE_ELEMS;
    v->n_obs = (double)n_obs;
    return SC_OK;
}
// Hermitian entry (i, j) of the bin record `rec` (conj: of its complex conjugate, the record of the mirrored bin): the stored
// upper triangle mirrored, the diagonal exactly real
__device__ inline double2 sc_csm_entry(ScRec rec, const ScCsmView& v, int i, int j, bool conj = false) {
    int ti = i >> 4, tj = j >> 4, ii = i & 15, jj = j & 15;
    const bool m = (ti > tj) || (ti == tj && ii > jj);
    if (m) { int t = ti; ti = tj; tj = t; t = ii; ii = jj; jj = t; }
    const int64_t off = (int64_t)sc_tile_index(ti, tj, v.NB) * SC_TILE_ELEMS + ii * 16 + jj;
    const double re = rec[(int64_t)v.p_csm * v.n_tiles * SC_TILE_ELEMS + off] / v.n_obs;
    double im = rec[(int64_t)(v.p_csm + 1) * v.n_tiles * SC_TILE_ELEMS + off] / v.n_obs;
    if (m) im = -im;
    if (conj) im = -im;
    if (i == j) im = 0.0;
    return make_double2(re, im);
}
// the record of accumulated bin `bin` of group g
__device__ inline ScRec sc_csm_record(ScRec accum, const ScCsmView& v, int64_t g, int64_t bin) {
    return accum + (g * v.F + bin) * v.floats_per_bin;
}
// S_g(n)[i][j] (two-sided bin n of group g)
__device__ inline double2 sc_csm_two_sided(ScRec accum, const ScCsmView& v, int64_t g, int64_t n, int i, int j) {
    int64_t bin = n;
    bool conj = false;
    if (!v.two_sided && n > v.N / 2) { bin = v.N - n; conj = true; }   // real input: S(-f) = conj S(f)
    return sc_csm_entry(sc_csm_record(accum, v, g, bin), v, i, j, conj);
}

// Lower Cholesky factor [[l00, 0], [l10, l11]] of the 2 x 2 lag-0 covariance [[r00, r01], [r01, r11]] of a pairwise Wilson problem;
// a covariance that is not positive definite gives the identity and (flag non-NULL) flags its batch: see k_init in sc_wilson.hip.
__device__ __forceinline__ void sc_lag0_cholesky2(double r00, double r11, double r01, double& l00, double& l10, double& l11,
                                                  int32_t* flag) {
    l00 = sqrt(r00); l10 = r01 / l00;
    const double t = r11 - l10 * l10;
    l11 = sqrt(t);
    const bool bad = !(r00 > 0.0) || !(t > 0.0);
    if (bad) { l00 = 1.0; l10 = 0.0; l11 = 1.0; }
    if (bad && flag) atomicOr(flag, 1);
}

// Workgroup-wide helpers of 256-thread kernels (sc_canonical.hip, sc_blockwise.hip).
// In-place lower Cholesky of the n x n Hermitian matrix L (row-major, row length ld, lower triangle valid), all 256 threads,
// right-looking; a pivot that is not positive is replaced by 1 and sets *bad.
__device__ inline void sc_wg_cholesky(double2* L, int ld, int n, int* bad) {
    const int tid = threadIdx.x;
    for (int k = 0; k < n; ++k) {
        if (tid == 0) {
            const double d = L[k * ld + k].x;
            if (!(d > 0.0)) *bad = 1;
            L[k * ld + k] = make_double2(sqrt(d > 0.0 ? d : 1.0), 0.0);
        }
        __syncthreads();
        const double dk = L[k * ld + k].x;
        for (int i = k + 1 + tid; i < n; i += 256) {
            const double2 v = L[i * ld + k];
            L[i * ld + k] = make_double2(v.x / dk, v.y / dk);
        }
        __syncthreads();
        const int m = n - k - 1;
        for (int e = tid; e < m * m; e += 256) {           // trailing lower triangle: L[i][j] -= L[i][k] conj(L[j][k]), k < j <= i
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) {
                const double2 a = L[i * ld + k], b = L[j * ld + k];
                const double2 t = make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
                double2 v = L[i * ld + j];
                v.x -= t.x; v.y -= t.y;
                L[i * ld + j] = v;
            }
        }
        __syncthreads();
    }
}
// block sum over 256 threads, two barriers (every thread gets the sum)
__device__ __forceinline__ double sc_wg_sum(double v, double* red4, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) red4[tid >> 6] = v;
    __syncthreads();
    const double r = red4[0] + red4[1] + red4[2] + red4[3];
    __syncthreads();
    return r;
}

// Decoding of group / observation indices into element offsets (see sc_spectra_desc).
struct ScAxes {
    int64_t sW, sR, sK, sF;
    int W, R, K, C, F;
    int kW, kR, kK;   // kept sizes (1 if reduced)
    int rW, rR, rK;   // reduced sizes (1 if kept)
    int n_groups, n_obs;
};

inline int sc_make_axes(const sc_spectra_desc* d, ScAxes* a) {
    if (!d) return SC_EINVAL;
    a->sW = d->stride_window; a->sR = d->stride_trial; a->sK = d->stride_taper; a->sF = d->stride_freq;
    a->W = (int)d->n_windows; a->R = (int)d->n_trials; a->K = (int)d->n_tapers;
    a->C = (int)d->n_signals; a->F = (int)d->n_freq;
    a->kW = d->reduce_window ? 1 : a->W; a->rW = d->reduce_window ? a->W : 1;
    a->kR = d->reduce_trial ? 1 : a->R;  a->rR = d->reduce_trial ? a->R : 1;
    a->kK = d->reduce_taper ? 1 : a->K;  a->rK = d->reduce_taper ? a->K : 1;
    a->n_groups = a->kW * a->kR * a->kK;
    a->n_obs = a->rW * a->rR * a->rK;
    return SC_OK;
}

__device__ inline int64_t sc_group_offset(const ScAxes& a, int g) {
    int gk = g % a.kK; g /= a.kK;
    int gr = g % a.kR; g /= a.kR;
    return (int64_t)g * a.sW + (int64_t)gr * a.sR + (int64_t)gk * a.sK;
}
__device__ inline int64_t sc_obs_offset(const ScAxes& a, int o) {
    int ok = o % a.rK; o /= a.rK;
    int orr = o % a.rR; o /= a.rR;
    return (int64_t)o * a.sW + (int64_t)orr * a.sR + (int64_t)ok * a.sK;
}

// Streaming stores of the spectra (written once, read by the next kernel from HBM: 6.5 GB at cfg3 against 32 MB of L2 and
// 256 MB of MALL): the non-temporal hint keeps the lines from lingering in the write-back L2 -- stage A 1.537 -> 1.471 ms at
// 256 samples, 1.517 -> 1.406 at 128, 2.186 -> 2.141 at 1024 (A/B inside one process, profiles/r03_stage_a_ab.txt).  ONLY for
// store groups that cover whole 128-byte lines: partial lines need the L2 to merge them (4096-sample windows, 32-byte
// pieces: 0.91 -> 1.73 ms with the hint; the float64 transform's 16-byte halves: 4.1 -> 6.1 ms).
#ifdef __HIPCC__
typedef float sc_f32x4 __attribute__((ext_vector_type(4)));
typedef float sc_f32x2 __attribute__((ext_vector_type(2)));
typedef double sc_f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sc_stream_store(float2* p, float2 a, float2 b) {          // 16-byte aligned pair
    const sc_f32x4 v = {a.x, a.y, b.x, b.y};
    __builtin_nontemporal_store(v, reinterpret_cast<sc_f32x4*>(p));
}
__device__ __forceinline__ void sc_stream_store(float2* p, float2 a) {
    const sc_f32x2 v = {a.x, a.y};
    __builtin_nontemporal_store(v, reinterpret_cast<sc_f32x2*>(p));
}
__device__ __forceinline__ void sc_stream_store(double2* p, double2 a) {
    const sc_f64x2 v = {a.x, a.y};
    __builtin_nontemporal_store(v, reinterpret_cast<sc_f64x2*>(p));
}
#endif
