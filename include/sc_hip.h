/* sc_hip.h -- C ABI of libsc_hip.so: the MI355X (gfx950) engine behind the
 * Multitaper / Connectivity API of Eden-Kramer-Lab/spectral_connectivity.
 *
 * This is the drop-in boundary for ONE path of the reference: time series ->
 * DPSS-tapered sliding-window FFT -> cross-spectral matrix -> expectation ->
 * coherence / PLI / wPLI / PLV / PPC (-> pairwise spectral Granger, canonical coherence;
 * delete-one jackknife standard errors of power, coherence and the phase-lag family;
 * the expectation-type measures of a few seed signals against a list of signals).
 * It replaces the reference's array-backend plug point, the import-time switch
 * `xp = cupy | numpy` plus `fft/ifft/...` (transforms.py:405-439, connectivity.py:31-65,
 * minimum_phase_decomposition.py:14-26), for the call sites listed per function below.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes.  Every `dev_*`/`d_*` pointer is DEVICE memory
 *    owned by the caller (the Python host allocates it with torch); the library never frees or
 *    retains caller buffers past the call.  Device memory the library allocates ITSELF, all of it
 *    released before the owning call returns or with the owning handle:
 *      - `sc_fft_plan` handles (sc_fft_plan_create*): the rocFFT plan, its work buffer and a <= 64 MB
 *        transform scratch (hipMalloc; freed by sc_fft_plan_destroy; sc_fft_plan_work_bytes reports it) -- the rocFFT plan
 *        object itself (twiddle tables, run-time compiled code: KBs to a few MB) is retired, not destroyed, and the
 *        Wilson kernels keep theirs for the life of the process: unloading rocFFT's code right before the first
 *        launch of another kernel has run stale instructions on MI355X / ROCm 7.0;
 *      - stream-ordered scratch (hipMallocAsync / hipFreeAsync on the call's stream) inside
 *        sc_multitaper_fft_f32 for N = 4096 (row-major spectra before the transpose, <= 2 GB),
 *        sc_canonical_coherence_f64 (inverted group factors, n_bins * n_groups * 4 KB; groups beyond 32 channels:
 *        the blocks of the pairs in flight, <= 192 MB),
 *        sc_global_coherence_f64 above 64 signals (rotation log; above 128 signals also the packed matrices) and the
 *        rocFFT work buffers of
 *        sc_granger_pairwise_f64 / sc_wilson_factor_f64 / sc_mvar_factor_f64 for lengths their fused
 *        transform kernel does not take.
 *      - sc_accumulate_f64: one side stream per device (created on first use, kept) and two events per call (destroyed
 *        when it returns) -- it forks its per-observation plane kernels from the caller's stream and joins them back
 *        before it returns --, and a stream-ordered scratch of (S - 1) records (<= 2 GB) for the partial sums of the S
 *        workgroups that share a bin's observations (hipMallocAsync / hipFreeAsync on `stream`).
 *      - sc_global_coherence_f64 beyond 64 signals: the matrices (n_signals^2 x 16 B per resident workgroup, <= 1024 of
 *        them) and per-vector work arrays of its eigen-solver (hipMalloc / hipFree inside the call, which synchronises).
 *    Everything else (spectra, records, workspaces, outputs) is caller memory with sizes the
 *    *_bytes / sc_accum_layout queries report.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All calls are
 *    asynchronous on that stream; nothing synchronises the device.
 *  - Return value: 0 on success, negative SC_E* otherwise; sc_last_error() returns a
 *    thread-local message for the last failure.
 *  - One plan / one stream is used by one host thread at a time; different streams may be
 *    driven from different threads.
 *
 * Device layouts (row-major, last index fastest)
 *  - time series      x[T][R][C]                      float   (reference layout, transforms.py:574)
 *  - tapers           h[K][L]                         float   (= reference tapers^T / fs, see sc_taper_windows_f32)
 *  - tapered windows  y[N][W][R][K][C]                float   (time-major: lanes <-> channels)
 *  - spectra          X[F][W][R][K][C]                float2  (one-sided, F = N/2+1) -- or any
 *                     layout described by sc_spectra_desc strides (e.g. the reference's
 *                     own (W,R,K,N,C) order for uploaded coefficients)
 *  - accumulators     A[bin][plane][tile][16][16]     float (double when SC_RECORD_F64 is set in `planes`: the
 *                     float64 engine)   bin = group*F + f ; upper-triangular
 *                     16x16 channel tiles (bi <= bj), tile index = bi*NB - bi*(bi-1)/2 + (bj-bi);
 *                     UN-normalised sums over observations (so trial shards can be summed)
 *  - measures         M[bin][C][C]                    float (or float2 for complex measures)
 */
#ifndef SC_HIP_H
#define SC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 8

/* error codes */
#define SC_OK 0
#define SC_EINVAL (-1)   /* bad argument / shape                 */
#define SC_EHIP (-2)     /* HIP runtime error (launch, memcpy)   */
#define SC_EFFT (-3)     /* rocFFT error                         */
#define SC_ENOMEM (-4)   /* work-buffer allocation failed        */
#define SC_EUNSUPPORTED (-5)

/* detrend_type of sc_taper_windows_f32 (transforms.py:1798-1915) */
#define SC_DETREND_NONE 0
#define SC_DETREND_CONSTANT 1
#define SC_DETREND_LINEAR 2

/* accumulator planes (bit mask).  Plane order inside a bin record is the order below,
 * skipping planes that are not requested.  CSM always occupies two planes (re, im). */
#define SC_PLANE_CSM 0x01u      /* sum X_i conj(X_j)            : 2 planes (re, im)  connectivity.py:447-461 */
#define SC_PLANE_ABS_IM 0x02u   /* sum |Im s|                   : 1 plane            connectivity.py:1008-1014 */
#define SC_PLANE_IM_SQ 0x04u    /* sum (Im s)^2                 : 1 plane            connectivity.py:1096-1102 */
#define SC_PLANE_SIGN_IM 0x08u  /* sum sign(Im s)               : 1 plane            connectivity.py:970-980 */
#define SC_PLANE_UNIT 0x10u     /* sum s/|s|                    : 2 planes (re, im)  connectivity.py:899-903 */
/* record format flag, OR-ed into `planes` wherever accumulator records are handed to a consumer (sc_measure_*,
 * sc_granger_pairwise_f64, sc_mvar_factor_f64, sc_global_coherence_f64, sc_canonical_coherence_f64): the records
 * hold doubles (written by sc_accumulate_f64) instead of floats */
#define SC_RECORD_F64 0x100u

/* measures of sc_measure_f32 (all on non-negative frequency bins the caller accumulated) */
#define SC_M_POWER 0                 /* connectivity.py:612-630   out float [bin][C]        */
#define SC_M_CSM 1                   /* connectivity.py:463-492   out float2 [bin][C][C]    */
#define SC_M_COHERENCY 2             /* connectivity.py:632-657   out float2                */
#define SC_M_COHERENCE_MAGNITUDE 3   /* connectivity.py:675-702   out float                 */
#define SC_M_COHERENCE_PHASE 4       /* connectivity.py:659-673                             */
#define SC_M_IMAGINARY_COHERENCE 5   /* connectivity.py:704-743                             */
#define SC_M_PLV 6                   /* connectivity.py:905-931   needs SC_PLANE_UNIT       */
#define SC_M_PLI 7                   /* connectivity.py:933-980   needs SC_PLANE_SIGN_IM    */
#define SC_M_WPLI 8                  /* connectivity.py:982-1028  needs CSM + ABS_IM        */
#define SC_M_DEBIASED_PLI2 9         /* connectivity.py:1030-1058 needs SIGN_IM             */
#define SC_M_DEBIASED_WPLI2 10       /* connectivity.py:1060-1127 needs CSM+ABS_IM+IM_SQ    */
#define SC_M_PPC 11                  /* connectivity.py:1129-1159 needs UNIT                */
#define SC_M_PLV_COMPLEX 12          /* connectivity.py:897-903   out float2                */

typedef struct sc_fft_plan sc_fft_plan; /* opaque */

/* How the (window, trial, taper) axes of the spectra map to memory and which of them the
 * expectation averages (connectivity.py:67-75 EXPECTATION).  Strides are in complex
 * elements; the channel stride is 1. */
typedef struct sc_spectra_desc {
    int64_t n_freq;      /* F: number of frequency bins to process                    */
    int64_t n_windows;   /* W */
    int64_t n_trials;    /* R */
    int64_t n_tapers;    /* K */
    int64_t n_signals;   /* C */
    int64_t stride_freq; /* elements between consecutive bins                          */
    int64_t stride_window;
    int64_t stride_trial;
    int64_t stride_taper;
    int32_t reduce_window; /* 1 if the expectation averages over windows ("time")     */
    int32_t reduce_trial;
    int32_t reduce_taper;
    int32_t reserved;
} sc_spectra_desc;

/* ---- library ------------------------------------------------------------------------ */
int sc_abi_version(void);
const char* sc_last_error(void);
int sc_device_count(int* count);

/* ---- stage A: window extraction + detrend + taper multiply (custom HIP) ---------------
 * Replaces _sliding_window (transforms.py:1311-1374), detrend (:1798-1915) and the taper
 * broadcast-multiply of _multitaper_fft (:1402-1404), fused, no window copy.
 *   y[w][r][k][c][n] = (x[w*step+n][r][c] - trend) * h[k][n]   for n <  min(L, N)
 *                    = 0                                        for min(L,N) <= n < N
 * (one row of N samples per transform, n fastest: the layout rocFFT streams at full rate)
 * The caller folds the reference's sqrt(fs) taper scaling and the 1/fs of
 * transforms.py:1405 into h (h = tapers^T / fs). */
int sc_taper_windows_f32(const float* d_x, int64_t T, int64_t R, int64_t C,
                         int64_t L, int64_t step, int64_t W, int64_t N,
                         const float* d_tapers, int64_t K, int detrend_type,
                         float* d_y, void* stream);
/* float64 engine: the reference's own precision (it promotes every input to float64, transforms.py:1402-1405) */
int sc_taper_windows_f64(const double* d_x, int64_t T, int64_t R, int64_t C,
                         int64_t L, int64_t step, int64_t W, int64_t N,
                         const double* d_tapers, int64_t K, int detrend_type,
                         double* d_y, void* stream);

/* float64 time series [T][R][C] -> the float32 copy [T][R][C_out] the float32 engine transforms (C_out >= C: channels
 * beyond C are zero, the pad channel of odd counts).  remove_mean != 0 subtracts the per-(trial, channel) mean over time
 * in float64 BEFORE the cast -- every window's detrend (transforms.py:1798-1915) removes any constant anyway, so only the
 * rounding changes: a DC offset many times the signal no longer costs the float32 copy its digits. */
int sc_timeseries_to_f32(const double* d_x, int64_t T, int64_t R, int64_t C, int remove_mean, float* d_y,
                         int64_t C_out, void* stream);

/* ---- stage A: batched real-to-complex FFT (rocFFT) -----------------------------------
 * Replaces fft(projected, n=N, axis=-2) of transforms.py:1405 (scipy.fft / cupyx.scipy.fft).
 * Input  y[batch][N] float (the rows sc_taper_windows_f32 writes), output X[F][batch] float2
 * (F = N/2+1, frequency-major like every spectra tensor here).  The plan transforms the rows in
 * unit-stride chunks into a scratch it owns (64 MB, cache-resident) and a tiled transpose moves
 * each chunk into X, zeroing the imaginary part of the DC / Nyquist rows on the way;
 * sc_fft_plan_work_bytes reports the device memory the plan holds. */
int sc_fft_plan_create(sc_fft_plan** plan, int64_t N, int64_t batch);
int sc_fft_plan_work_bytes(const sc_fft_plan* plan, size_t* bytes);
int sc_fft_execute(sc_fft_plan* plan, const float* d_y, void* d_X /*float2*/, void* stream);
int sc_fft_plan_destroy(sc_fft_plan* plan);
/* double-precision plans of the float64 engine: y double rows in, X[F][batch] double2 out */
int sc_fft_plan_create_f64(sc_fft_plan** plan, int64_t N, int64_t batch);
int sc_fft_execute_f64(sc_fft_plan* plan, const double* d_y, void* d_X /*double2*/, void* stream);

/* ---- stage A, fused fast path (custom HIP) ---------------------------------------------
 * Window extraction + detrend + taper multiply + real FFT + transposed store in ONE kernel:
 * replaces _sliding_window, detrend, _multitaper_fft and the swapaxes of Multitaper.fft
 * (transforms.py:1147-1171, :1311-1405) with a single read of x and a single write of
 *   X[f][w][r][k][c],  f = 0..N/2   (one-sided; the negative bins of a real input are
 *                                    conjugate mirrors and are never materialised).
 * Supported when sc_multitaper_fft_supported(L, N) != 0: L <= N and N either a power of two in
 * 64 ... 4096 (register-resident radix-16 passes; from 256 samples on, when the request fills the chip, two half-workgroups
 * in anti-phase -- one runs the passes while the other stores: sc_mtfft_long.hip) or 2^a 3^b 5^c in 8 ... 2048 (mixed-radix Stockham
 * passes in LDS: the lengths next_fast_len, transforms.py:1024-1036, returns for the usual window
 * durations -- 200, 250, 500, 1000 ...); otherwise use sc_taper_windows_f32 + sc_fft_execute
 * (rocFFT, any length).
 * d_twiddles: float2[N] device table filled once by sc_fft_twiddles_f32(N, ...). */
int sc_multitaper_fft_supported(int64_t L, int64_t N);
int sc_fft_twiddles_f32(int64_t N, void* d_twiddles /*float2[N]*/, void* stream);
int sc_multitaper_fft_f32(const float* d_x, int64_t T, int64_t R, int64_t C,
                          int64_t L, int64_t step, int64_t W, int64_t N,
                          const float* d_tapers, int64_t K, int detrend_type,
                          const void* d_twiddles, void* d_X /*float2*/, void* stream);
/* float64 engine, the same fusion in doubles (sc_mtfft_f64.hip): complex128 spectra X[f][w][r][k][c]; powers of two
 * 64 ... 1024: register-resident radix-16 passes like the float32 kernel; the next_fast_len lengths: one wave per
 * packed channel pair, in-place mixed-radix passes in LDS; twiddles computed by the kernel.  Lengths with a compiled
 * transform: 64, 128, 256, 512, 1024 and 200, 250, 400, 500, 1000 (sc_multitaper_fft_f64_supported); every other
 * length: sc_taper_windows_f64 + sc_fft_execute_f64. */
int sc_multitaper_fft_f64_supported(int64_t L, int64_t N);
int sc_multitaper_fft_f64(const double* d_x, int64_t T, int64_t R, int64_t C,
                          int64_t L, int64_t step, int64_t W, int64_t N,
                          const double* d_tapers, int64_t K, int detrend_type,
                          void* d_X /*double2*/, void* stream);

/* ---- stage B: accumulators -----------------------------------------------------------
 * Number of floats of one bin record for `planes`, and total bins (groups * F). */
int sc_accum_layout(const sc_spectra_desc* desc, uint32_t planes,
                    int64_t* n_bins, int64_t* floats_per_bin, int64_t* n_groups,
                    int64_t* n_observations);

/* Sum over the averaged axes of the per-observation cross-spectral outer product, on the
 * matrix cores (v_mfma_f32_16x16x4_f32), upper-triangular 16x16 tiles only.
 * Replaces _complex_inner_product + mean of connectivity.py:447-492, :1799-1822 without
 * materialising the per-observation (W,R,K,N,C,C) temporary.  Writes the two CSM planes
 * of every bin record in d_accum (other planes untouched).  Sums are UN-normalised: a rank
 * that holds a shard of the trials accumulates its shard and the records are added. */
int sc_csm_accumulate_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc,
                          uint32_t planes, float* d_accum, void* stream);

/* Per-observation non-linear planes (|Im s|, (Im s)^2, sign Im s, s/|s|), VALU kernel.
 * Replaces the fcn hook of _expectation_cross_spectral_matrix (connectivity.py:463-492)
 * as used by PLV/PLI/wPLI/debiased variants/PPC (:897-1159).  Writes the requested
 * non-CSM planes of every bin record. */
int sc_nonlinear_accumulate_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc,
                                uint32_t planes, uint32_t which, float* d_accum, void* stream);

/* Fused stage B for the headline pair coherence + wPLI (planes = CSM | ABS_IM; CSM alone is accepted too and
 * then only the matrix-core update runs): ONE pass over the spectra computes
 * the CSM planes AND the per-observation Im(x_i conj x_j) products of the ABS_IM plane on the bf16 matrix
 * pipe (exact 3-way bf16 split of every f32 coefficient; 12-wave workgroups: one CSM wave and two |Im| waves
 * per SIMD over one double-buffered LDS staging of the spectra, rows pulled HBM -> LDS directly).  Same results as
 * sc_csm_accumulate_f32 + sc_nonlinear_accumulate_f32(SC_PLANE_ABS_IM); even n_signals <= 256 (above 128 channels
 * the record is filled by several launches over 64-channel quarters: the two 128-channel halves, then every quarter
 * of the first half against every quarter of the second). */
int sc_fused_supported(int64_t n_signals);
int sc_fused_csm_absim_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc,
                           uint32_t planes, float* d_accum, void* stream);
/* Same, with a device workspace (sc_fused_workspace_bytes; may be 0) that lets several workgroups share
 * one (window, frequency) bin when the bin count does not fill the GPU's compute units evenly: each
 * sums part of the observations into its own record, folded together in a fixed order afterwards. */
int64_t sc_fused_workspace_bytes(const sc_spectra_desc* desc, uint32_t planes);
int sc_fused_csm_absim_ws_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, uint32_t planes,
                              float* d_accum, void* d_workspace, int64_t workspace_bytes, void* stream);

/* SC_PLANE_UNIT of the record, sum over observations of s/|s| (phase_locking_value,
 * pairwise_phase_consistency: connectivity.py:897-981), through the same kernels: s/|s| factorises into
 * (x_i/|x_i|) conj(x_j/|x_j|), so the sum is the cross-spectral matrix of the unit phasors x/|x|
 * (0/0 -> NaN like the reference's x/abs(x)).  The normalisation happens while the rows are staged, in both kernels:
 * no copy of the spectra, d_scratch / scratch_bytes are ignored and sc_fused_unit_scratch_bytes returns 0 (both kept
 * for ABI v2 callers).  Shapes, workspace and split as above. */
/* SC_PLANE_UNIT for shapes the one-pass kernels do not take (odd channel counts without a pad channel): a normalised copy of the
 * spectra (x/|x|, 0 -> NaN) in d_scratch (sc_unit_scratch_bytes) goes through the f32-MFMA CSM kernel. */
int64_t sc_unit_scratch_bytes(const sc_spectra_desc* desc);
int sc_unit_accumulate_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, uint32_t planes,
                           float* d_accum, void* d_scratch, int64_t scratch_bytes, void* stream);

/* Which planes of `planes` the one-pass entry points fill for this shape (even n_signals <= 256): CSM, |Im s| (with
 * CSM) and s/|s|; (Im s)^2 (with CSM and |Im s|, filled by sc_fused_csm_absim_ws_f32: in the same pass up to 52 channels,
 * as a second pass of the matrix-core kernel above) and sign(Im s) (sc_fused_sign_ws_f32: phase_lag_index,
 * connectivity.py:933-980; f32 VALU kernel up to 40 channels, above it a pass of the matrix-core kernel whose |Im| waves
 * sum sign(d) of the per-observation products).  Whatever is left is sc_nonlinear_accumulate_f32's. */
uint32_t sc_fused_planes_covered(const sc_spectra_desc* desc, uint32_t planes);
int sc_fused_sign_ws_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, uint32_t planes,
                         float* d_accum, void* d_workspace, int64_t workspace_bytes, void* stream);
int64_t sc_fused_unit_scratch_bytes(const sc_spectra_desc* desc);
int sc_fused_unit_ws_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, uint32_t planes,
                         float* d_accum, void* d_workspace, int64_t workspace_bytes, void* d_scratch,
                         int64_t scratch_bytes, void* stream);

/* ---- planes format (ABI v4): every real number stored as two f16 pieces, x * scale[c] = h + m ---------------------------
 * The one-pass stage-B kernels multiply on the 16-bit matrix pipe and split every f32 coefficient while they stage it; stage A
 * can store the pieces instead (sc_multitaper_fft_planes_f32): stage B's staging becomes plain HBM -> LDS loads and its
 * products need three cross terms instead of six.  h = f16(x scale), m = f16(x scale - h): 22 significant bits; scale[c] is
 * a power of two per channel that keeps every coefficient inside the f16 range (sc_planes_scales_*); records come out
 * unscaled (exactly: powers of two).  Layout: dense rows [F][W][R][K] (bin, window, trial, taper) of
 * sc_planes_row_bytes(C) = 256 * ceil(C / 32) bytes: [channel tile of 32][plane Re h, Re m, Im h, Im m][32 channels] f16,
 * absent channels zero -- 8 bytes per coefficient, like the complex64 spectra of _multitaper_fft (transforms.py:1377-1405).
 * d_scale: float[2 C] = the scales, then their reciprocals. */
int64_t sc_planes_row_bytes(int64_t n_signals);
/* scales from a bound on the spectra of a (T, R, C) time series: |X_k(f)| <= 8 max|x| * taper_abs_sum, taper_abs_sum =
 * max_k sum_n |tapers[k][n]| (the tapers as passed to stage A, i.e. / fs); d_work: 4 C bytes of device scratch */
int sc_planes_scales_from_series_f32(const float* d_x, int64_t T, int64_t R, int64_t C, double taper_abs_sum,
                                     float* d_scale, void* d_work, void* stream);
/* The same scan with the QUALITY CHECK of the format.  One scale per channel serves every window, so the format delivers its 22
 * bits only while a channel's typical coefficient stays well above the f16 subnormals in scaled units -- which a DC offset or an
 * artefact thousands of times the typical amplitude would prevent.  This form (a) takes the scale from the RANGE of the channel
 * when stage A detrends (detrend_type != 0: |x - trend| <= 4 (max x - min x), a DC offset no longer enters; without detrend
 * |x| <= max |x|), and (b) reports *d_quality (device float) = min over the channels of (typical sample magnitude: the standard
 * deviation -- root mean square without detrend -- of the channel's QUIETEST slab of >= 128 consecutive (time, trial) rows) * scale.  The typical coefficient in scaled units is that times
 * min_k ||tapers_k||_2; below SC_PLANES_MIN_TYPICAL the host keeps complex64 spectra (sc_multitaper_fft_f32) -- the planes
 * format is a device detail, never a precision trade.  d_work: sc_planes_scales_work_bytes(T * R, C) bytes. */
#define SC_PLANES_MIN_TYPICAL 2.5f
int64_t sc_planes_scales_work_bytes(int64_t n_rows, int64_t width);
int sc_planes_scales_quality_f32(const float* d_x, int64_t T, int64_t R, int64_t C, int detrend_type, double taper_abs_sum,
                                 float* d_scale, void* d_work, int64_t work_bytes, float* d_quality, void* stream);
/* scales from the largest |Re|, |Im| of dense complex64 rows [n_rows][C] */
int sc_planes_scales_from_spectra_f32(const void* d_X /*float2*/, int64_t n_rows, int64_t C, float* d_scale, void* d_work,
                                      void* stream);
/* Stage A straight into the planes format: sc_multitaper_fft_f32 with the spectra leaving as f16 pieces (same transform,
 * same coefficients up to the 22-bit representation; window lengths N = 64 ... 4096, powers of two, even n_signals). */
int sc_multitaper_fft_planes_supported(int64_t L, int64_t N, int64_t n_signals);
int sc_multitaper_fft_planes_f32(const float* d_x, int64_t T, int64_t R, int64_t C, int64_t L, int64_t step, int64_t W,
                                 int64_t N, const float* d_tapers, int64_t K, int detrend_type, const void* d_twiddles,
                                 const float* d_scale, void* d_P, void* stream);
/* complex64 spectra described by desc (strides in elements) <-> planes buffer (dense rows, desc's sizes) */
int sc_planes_from_spectra_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, const float* d_scale, void* d_P,
                               void* stream);
int sc_spectra_from_planes_f32(const void* d_P, const sc_spectra_desc* desc, const float* d_scale, void* d_X /*float2*/,
                               void* stream);
/* Stage B on the planes format: the CSM planes and the |Im s| plane of every bin record in one pass, exactly what
 * sc_fused_csm_absim_ws_f32 writes (replaces _expectation_cross_spectral_matrix with fcn = identity and abs(Im),
 * connectivity.py:463-526, :982-1028).  desc: sizes and reduce flags (strides ignored: the rows are dense).  Takes
 * planes == SC_PLANE_CSM, SC_PLANE_CSM | SC_PLANE_ABS_IM, the latter | SC_PLANE_IM_SQ (debiased wPLI: a second pass squares
 * the per-observation products) or SC_PLANE_SIGN_IM alone (phase_lag_index: connectivity.py:933-980); up to 1024 signals
 * (129 and more in several launches over 32-channel blocks; more than 256: round 6); observations of a bin that form one linear run of rows (every
 * expectation type but "time_tapers" with several trials); sc_fused2_supported tells.
 * Workspace as for sc_fused_csm_absim_ws_f32 (sc_fused_workspace_bytes with the same desc). */
int sc_fused2_supported(const sc_spectra_desc* desc, uint32_t planes);
/* The same without the pass that folds the split-bin partial records: *n_parts workgroups shared every bin; part 0 of the
 * records is in d_accum, part k >= 1 at (float*)d_workspace + (k - 1) * n_bins * floats_per_bin (sc_accum_layout) -- for
 * sc_measure_multi_parts, which sums them while it reads. */
int sc_fused2_csm_absim_parts_f32(const void* d_P, const sc_spectra_desc* desc, const float* d_scale, uint32_t planes,
                                  float* d_accum, void* d_workspace, int64_t workspace_bytes, int* n_parts, void* stream);
/* shader clock (GHz) the device sustained during the last sc_fused2_csm_absim_f32 launch (in-kernel cycle / real-time counters) */
int sc_debug_fused2_clock(double* ghz);
/* The diagnostic switches of the library (SC_FUSED_DEBUG, SC_FUSED_SPLIT, SC_FUSED_SPLIT_TAIL, SC_MTFFT_DEBUG, SC_WILSON_FFT, ...: ablation tools and
 * the tests of alternative kernels) are environment variables read once when the library is loaded; a host that changes one
 * afterwards calls this to have them read again.  No reference counterpart (the reference has no native code). */
int sc_debug_reload_env(void);
/* rocFFT plans are never destroyed (a destroyed plan unloads run-time compiled code that a lazily loaded kernel of this library
 * has then executed stale: see sc_fft_plan_destroy); they live in pools keyed by geometry and are re-used.  *n_created:
 * rocfft_plan_create calls of the process; *n_pooled: plans the pools hold; *n_idle: of those, real-to-complex row plans that
 * belong to no live sc_fft_plan.  n_created == n_pooled always: what a process holds is bounded by the DISTINCT (length, batch,
 * precision) geometries it has asked for, not by how many sc_fft_plan objects it created and destroyed.  Any pointer may be NULL. */
int sc_debug_fft_plans(int64_t* n_created, int64_t* n_pooled, int64_t* n_idle);
int sc_fused2_csm_absim_f32(const void* d_P, const sc_spectra_desc* desc, const float* d_scale, uint32_t planes,
                            float* d_accum, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- stage C: measures epilogue ------------------------------------------------------
 * Elementwise measure algebra on accumulated sums (connectivity.py:612-1159): divides by
 * n_observations AFTER any cross-GPU reduction, applies the reference's eps clamps, NaN /
 * zero diagonals and clips, mirrors the triangle into the full C x C matrix.
 * d_out: float [n_bins][C][C] (float2 for complex measures, float [n_bins][C] for power). */
int sc_measure_f32(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                   int64_t n_observations, int measure, void* d_out, void* stream);
/* The same measures written as double / double2 -- what the reference returns (float64 / complex128) -- from float
 * or (SC_RECORD_F64) double records: no widening pass over the result. */
int sc_measure_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                   int64_t n_observations, int measure, void* d_out, void* stream);
/* Up to SC_MEASURE_MULTI_MAX real-valued C x C measures (coherence magnitude / phase, imaginary coherence, PLV, PPC,
 * PLI, wPLI and the debiased variants) of ONE record in one launch: the record is read once.  measures, d_outs: HOST
 * arrays of n_measures entries; d_outs[m]: float (_f32) or double (_f64) [n_bins][C][C]. */
#define SC_MEASURE_MULTI_MAX 4
int sc_measure_multi_f32(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                         int64_t n_observations, int n_measures, const int* measures, void* const* d_outs,
                         void* stream);
int sc_measure_multi_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                         int64_t n_observations, int n_measures, const int* measures, void* const* d_outs,
                         void* stream);
/* The same, from a record that arrives as n_parts partial records (float, or double with SC_RECORD_F64 in `planes`): part 0
 * at d_part0, part k >= 1 at d_rest + (k - 1) * part_stride elements -- the bin blocks a rank received from the other ranks
 * in the direct exchange of the trial-sharded path (the sum over trial shards), or the per-workgroup partial
 * records of a split-bin stage B (sc_fused2_csm_absim_parts_f32).  The parts are summed in part order in the records'
 * precision while they are read: no summation pass, no second copy of the record.  wide: float64 outputs. */
int sc_measure_multi_parts(const void* d_part0, const void* d_rest, int n_parts, int64_t part_stride, int64_t n_bins,
                           int64_t n_signals, uint32_t planes, int64_t n_observations, int n_measures, const int* measures,
                           void* const* d_outs, int wide, void* stream);
/* ONE measure of sc_measure_f32 / _f64 -- power and the complex-valued ones included -- from partial records (same layout);
 * wide != 0: double / complex128 output. */
int sc_measure_parts(const void* d_part0, const void* d_rest, int n_parts, int64_t part_stride, int64_t n_bins,
                     int64_t n_signals, uint32_t planes, int64_t n_observations, int measure, void* d_out, int wide, void* stream);

/* ---- stage B of the float64 engine -----------------------------------------------------
 * Replaces the same reference code as sc_csm_accumulate_f32 / sc_nonlinear_accumulate_f32 (connectivity.py:447-526,
 * :897-1159, :1799-1822) in the reference's own arithmetic: complex128 spectra (any sc_spectra_desc layout, 16-byte
 * aligned), the cross-spectral matrix on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), the per-observation planes on
 * the fp64 VALU, double records of the same tile layout.  `which` names the planes to fill (subset of `planes`).
 * Selected by Connectivity(dtype=numpy.complex128), the reference's default dtype. */
int sc_accumulate_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, uint32_t planes, uint32_t which,
                      double* d_accum, void* stream);

/* ---- timing ------------------------------------------------------------------------------
 * hipEvent timers inside the library: after sc_timing_enable(1) every compute entry point brackets its launches with
 * two events on the stream it was given; sc_last_timing waits for them, writes (name, milliseconds) in call order
 * (at most max_entries) and forgets them.  sc_timing_enable(0) stops recording.  One timing session per process. */
typedef struct sc_timing {
    char name[48];
    float ms;
} sc_timing;
int sc_timing_enable(int on);
int sc_last_timing(sc_timing* out, int max_entries, int* n_entries);

/* ---- pairwise spectral Granger prediction (batched 2x2 Wilson factorisation, fp64) -----
 * Replaces Connectivity.pairwise_spectral_granger_prediction / subset_... and the Python
 * loop over pairs of _estimate_spectral_granger_prediction (connectivity.py:1161-1213,
 * :2282-2340) together with minimum_phase_decomposition (minimum_phase_decomposition.py:
 * 227-322), _estimate_transfer_function / _estimate_noise_covariance /
 * _remove_instantaneous_causality / _estimate_predictive_power (connectivity.py:1679-1779,
 * :1825-1848).  All (group, pair) problems advance together; FFTs along frequency are rocFFT
 * batched Z2Z plans created inside the call.
 *   d_accum     accumulator records with SC_PLANE_CSM, n_groups * n_freq_accum bins;
 *               n_freq_accum = N/2+1 (real input: negative bins are mirrored) or N.
 *   d_pairs     int32 [n_pairs][2] channel indices (i, j)
 *   d_out       double [n_groups][N/2+1][C][C]; out[.., i, j] = influence j -> i, NaN
 *               elsewhere (diagonal, pairs not requested, non-positive values)
 *   d_n_iter    int32 [n_groups*n_pairs] Wilson iterations used per problem
 *   d_status    int32 [n_groups*n_pairs]: 1 converged, 0 hit max_iter
 *   h_summary   optional HOST int32[3]: {iterations run, problems not converged, problems restarted because a lag-0
 *               covariance of their batch was not positive definite}.  The reference's batched Cholesky fails as a
 *               whole: every window of the channel pair then starts from the Cholesky factor of a random Wishart
 *               draw around a multiple of the identity (minimum_phase_decomposition.py:78-93, global NumPy generator);
 *               here every (group, pair) problem of such a pair starts from its expectation, the identity -- the
 *               start matters, the fixed point reached at a finite N depends on it (tests/golden/f12_*).
 *   flags       SC_GRANGER_KEEP_OUTPUT: do not NaN-fill d_out first (the caller walks a long pair list in chunks
 *               that share one output; any number of (group, pair) problems is accepted per call, the workspace
 *               is what grows: n_groups * n_pairs * N * 160 bytes)
 * Unlike every other entry point this one SYNCHRONISES the stream, once per four Wilson iterations (to stop
 * when every problem has converged, like the reference loop; converged problems are skipped by every kernel,
 * so the iterations queued past the last convergence are empty launches). */
#define SC_GRANGER_KEEP_OUTPUT 1
int sc_granger_workspace_bytes(int64_t n_groups, int64_t n_pairs, int64_t N, size_t* bytes);
int sc_granger_pairwise_f64(const void* d_accum, int64_t n_groups, int64_t n_freq_accum,
                            int64_t N, int64_t n_signals, uint32_t planes, int64_t n_observations,
                            const int32_t* d_pairs, int64_t n_pairs, double tolerance, int max_iterations,
                            void* d_work, size_t work_bytes, int flags, double* d_out, int32_t* d_n_iter,
                            int32_t* d_status, int32_t* h_summary, void* stream);

/* Minimum-phase (Wilson) factor of caller-supplied two-sided 2x2 Hermitian spectra: replaces
 * minimum_phase_decomposition() (minimum_phase_decomposition.py:227-322) for c <= 2 (a 1x1
 * spectrum is embedded as diag(s, 1)).  d_S: double [P][4][N] = (s00, s11, Re s01, Im s01) per bin;
 * d_G: complex128 [P][4][N] = (g00, g01, g10, g11), S = G G^H.  Workspace as for n_groups = 1,
 * n_pairs = P of sc_granger_workspace_bytes.  h_summary: HOST int32[3] as above.  Synchronises the stream (see above). */
int sc_wilson_factor_f64(const double* d_S, int64_t n_problems, int64_t N, double tolerance,
                         int max_iterations, void* d_work, size_t work_bytes, void* d_G /*complex128*/,
                         int32_t* d_n_iter, int32_t* d_status, int32_t* h_summary, void* stream);

/* ---- full C x C Wilson factor and the directed MVAR measures (fp64) ----------------------
 * Replaces Connectivity._minimum_phase_factor / _transfer_function / _noise_covariance /
 * _MVAR_Fourier_coefficients (connectivity.py:567-589), minimum_phase_decomposition() for any c
 * (minimum_phase_decomposition.py:227-322) and directed_transfer_function, directed_coherence,
 * partial_directed_coherence, generalized_partial_directed_coherence,
 * direct_directed_transfer_function (connectivity.py:1237-1426).  All windows iterate together,
 * converged windows are frozen; up to 128 signals the C x C factor of one (window, bin) lives in the registers of one
 * workgroup, 129 ... 512 run a panel-blocked inverse in global memory and products cut into 128 x 128 blocks:
 * n_signals <= sc_mvar_max_signals() (512 since round 6; records of more than 256 signals come from the planes-format
 * stage B or are assembled from channel-block pairs by the host), larger systems return SC_EUNSUPPORTED.
 * sc_mvar_factor_f64: exactly one of d_accum (accumulator records holding SC_PLANE_CSM, N or N/2+1
 * bins per window, real-input symmetry completes the rest) and d_S (complex128 [P][N][C][C], two-sided
 * Hermitian spectra) is non-NULL.  d_G: complex128 [P][N][C][C].  d_status[p]: 1 converged, 0 not
 * converged after max_iterations; h_summary = HOST int32[3] {iterations run, windows still running, windows whose
 * lag-0 covariance was not positive definite and that started from the identity (see sc_granger_pairwise_f64)}.
 * Synchronises the stream once per four iterations.  Per iteration: A = G^-1 S G^-H + I by a register-resident
 * Gauss-Jordan elimination per (window, bin) -- of [G | S] up to 64 signals; of G alone, followed by two matrix-core
 * products, for 65 ... 128 (five instead of three C^2 N complex128 arrays of workspace per window) --, the causal
 * transform pair along frequency, G <- G A+ on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).
 * sc_mvar_measure_f64: d_G as above -> double [P][N/2+1][C][C] (SC_MVAR_DTF..DDTF), complex128
 * [P][N/2+1][C][C] (SC_MVAR_TRANSFER, SC_MVAR_COEFFICIENTS) or double [P][C][C] (NOISE_COVARIANCE).
 * The Tikhonov terms are the reference's: 1e-12 * mean(H0^2) over all windows, 1e-12 * mean(|H|^2)
 * over all windows and non-negative bins.  One workspace size serves both calls. */
#define SC_MVAR_DTF 0                /* connectivity.py:1237-1270 */
#define SC_MVAR_DC 1                 /* connectivity.py:1272-1309 */
#define SC_MVAR_PDC 2                /* connectivity.py:1311-1364 */
#define SC_MVAR_GPDC 3               /* connectivity.py:1366-1400 */
#define SC_MVAR_DDTF 4               /* connectivity.py:1402-1426 */
#define SC_MVAR_TRANSFER 5           /* connectivity.py:1712-1748 */
#define SC_MVAR_COEFFICIENTS 6       /* connectivity.py:581-589   */
#define SC_MVAR_NOISE_COVARIANCE 7   /* connectivity.py:1679-1709 */
int sc_mvar_max_signals(void);
int sc_mvar_workspace_bytes(int64_t n_groups, int64_t n_signals, int64_t N, size_t* bytes);
int sc_mvar_factor_f64(const void* d_accum, const void* d_S /*complex128*/, int64_t n_groups,
                       int64_t n_freq_accum, int64_t N, int64_t n_signals, uint32_t planes,
                       int64_t n_observations, double tolerance, int max_iterations, void* d_work,
                       size_t work_bytes, void* d_G /*complex128*/, int32_t* d_n_iter, int32_t* d_status,
                       int32_t* h_summary, void* stream);
int sc_mvar_measure_f64(const void* d_G /*complex128*/, int64_t n_groups, int64_t N, int64_t n_signals,
                        int which, void* d_out, void* d_work, size_t work_bytes, void* stream);

/* ---- conditional spectral Granger prediction (ABI v7, fp64) --------------------------------
 * j -> i given every other signal (Geweke 1984; Ding, Chen & Bressler 2006, section 3.3); the reference raises
 * NotImplementedError (connectivity.py:1215-1224).  Needs the full factor d_G of sc_mvar_factor_f64 (complex128
 * [n_groups][N][C][C]) and factors, for every dropped signal j of d_dropped (int32 [n_dropped]), the spectrum with row and
 * column j removed by the same Wilson iteration (sc_mvar_factor_f64 on n_dropped * n_groups problems of C - 1 signals;
 * problem d * n_groups + g).  With Psi0 = Re mean_n Psi, Sigma = Psi0 Psi0^T and Phi0 / Sigma^r those of the reduced factor Phi:
 *     out[g][f][i][j] = ln(Sigma^r[i][i] Sigma[i][i] / |v_i(f)|^2),  v = Phi0 Phi(f)^-1 (Psi(f) Psi0^T)[rows != j, col i]
 * at the row of i in the reduced system, for every i != j; non-positive values are NaN.
 *   d_accum / d_S  exactly one: the records sc_mvar_factor_f64 takes (SC_PLANE_CSM, N or N/2+1 bins per group) or
 *                  complex128 [n_groups][N][C][C] two-sided Hermitian spectra
 *   d_out          double [n_groups][N/2+1][C][C]; NaN-filled first (diagonal, columns not dropped) unless flags has
 *                  SC_CONDITIONAL_KEEP_OUTPUT (the caller walks the dropped signals in chunks that share one output)
 *   d_n_iter, d_status  int32 [n_dropped * n_groups]: Wilson iterations / 1 converged, 0 hit max_iterations, per reduced problem
 *   h_summary      optional HOST int32[3] {iterations run, reduced problems not converged, identity starts}, as sc_mvar_factor_f64
 * n_dropped * n_groups <= 65535.  Workspace: sc_conditional_granger_workspace_bytes(n_groups, C, N, n_dropped): the reduced
 * spectra and factors (two complex128 arrays [n_dropped * n_groups][N][C-1][C-1]), the larger of the reduced factorisation's
 * workspace and the epilogue's two such arrays, and complex128 [n_groups][N/2+1][C][C].
 * 2 <= n_signals <= sc_mvar_max_signals(), otherwise SC_EUNSUPPORTED.  Synchronises the stream (as sc_mvar_factor_f64). */
#define SC_CONDITIONAL_KEEP_OUTPUT 1
int sc_conditional_granger_workspace_bytes(int64_t n_groups, int64_t n_signals, int64_t N, int64_t n_dropped, size_t* bytes);
int sc_conditional_granger_f64(const void* d_accum, const void* d_S /*complex128*/, int64_t n_groups, int64_t n_freq_accum,
                               int64_t N, int64_t n_signals, uint32_t planes, int64_t n_observations,
                               const void* d_G /*complex128*/, const int32_t* d_dropped, int64_t n_dropped, double tolerance,
                               int max_iterations, void* d_work, size_t work_bytes, int flags, double* d_out,
                               int32_t* d_n_iter, int32_t* d_status, int32_t* h_summary, void* stream);

/* ---- blockwise spectral Granger prediction (ABI v8, fp64) ----------------------------------
 * Block b -> block a for pairs of signal BLOCKS (Geweke 1982, multivariate form); the reference raises NotImplementedError
 * (connectivity.py:1226-1235).  (Signal groups are "blocks" here: n_groups is the records' groups, windows x kept axes.)
 * Pair q has m signals, d_members[q][0 .. n_a-1] of block a then d_members[q][n_a .. m-1] of block b (n_a = d_split[q]); its
 * m x m two-sided spectrum S of every group is factored by the Wilson iteration of sc_mvar_factor_f64 (problem q * n_groups + g).
 * With Psi0 = Re mean_n Psi, U_b an orthonormal basis of the null space of the rows Psi0[a, :] (U_a of Psi0[b, :]),
 * V_a = Psi[a, :](f) U_b and V_b = Psi[b, :](f) U_a:
 *     out[g][f][A][B] = ln det S_aa(f) - ln det(S_aa(f) - V_a V_a^H)      (B -> A; A, B = d_cell[q][0], d_cell[q][1])
 *     out[g][f][B][A] = ln det S_bb(f) - ln det(S_bb(f) - V_b V_b^H)      (A -> B)
 * = ln det S_aa - ln det(S_aa - H_ab Sigma~_bb H_ab^H), Sigma~_bb = Sigma_bb - Sigma_ba Sigma_aa^-1 Sigma_ab, H = Psi Psi0^-1,
 * Sigma = Psi0 Psi0^T; with n_a = n_b = 1 the pairwise measure.  A Cholesky pivot that is not positive, or a value <= 0, is NaN.
 *   d_accum / d_S  exactly one: the records sc_mvar_factor_f64 takes (SC_PLANE_CSM, N or N/2+1 bins per group) or
 *                  complex128 [n_groups][N][n_signals][n_signals] two-sided Hermitian spectra
 *   d_members      int32 [n_pairs][m], signals in [0, n_signals); d_split int32 [n_pairs], 1 <= n_a < m (n_a may differ inside a
 *                  batch); d_cell int32 [n_pairs][2], distinct output block indices in [0, n_blocks).  The three lists are read
 *                  back and checked before any launch.
 *   d_out          double [n_groups][N/2+1][n_blocks][n_blocks]; NaN-filled first (diagonal, pairs not computed) unless flags has
 *                  SC_BLOCKWISE_KEEP_OUTPUT (the caller walks the pairs in batches that share one output); only the two cells of
 *                  each pair are written
 *   d_n_iter, d_status  int32 [n_pairs * n_groups]: Wilson iterations / 1 converged, 0 hit max_iterations, per problem
 *   h_summary      optional HOST int32[3] {iterations run, problems not converged, identity starts}, as sc_mvar_factor_f64
 * 2 <= m <= sc_mvar_max_signals(), otherwise SC_EUNSUPPORTED; n_pairs * n_groups <= 65535.  Workspace:
 * sc_blockwise_granger_workspace_bytes(n_groups, m, N, n_pairs): the spectra and factors (two complex128 arrays
 * [n_pairs * n_groups][N][m][m]) and the larger of the factorisation's workspace and the epilogue's arrays (complex128
 * [n_pairs * n_groups][N/2+1][m][m] and two [n_pairs * n_groups][m][m]).  Synchronises the stream (as sc_mvar_factor_f64). */
#define SC_BLOCKWISE_KEEP_OUTPUT 1
int sc_blockwise_granger_workspace_bytes(int64_t n_groups, int64_t m, int64_t N, int64_t n_pairs, size_t* bytes);
int sc_blockwise_granger_f64(const void* d_accum, const void* d_S /*complex128*/, int64_t n_groups, int64_t n_freq_accum,
                             int64_t N, int64_t n_signals, uint32_t planes, int64_t n_observations, const int32_t* d_members,
                             const int32_t* d_split, const int32_t* d_cell, int64_t n_pairs, int64_t m, int64_t n_blocks,
                             double tolerance, int max_iterations, void* d_work, size_t work_bytes, int flags, double* d_out,
                             int32_t* d_n_iter, int32_t* d_status, int32_t* h_summary, void* stream);

/* ---- global coherence (fp64, from the accumulated CSM) --------------------------------------
 * Replaces Connectivity.global_coherence / _estimate_global_coherence (connectivity.py:822-895,
 * :2245-2279): the leading squared singular values / n_estimates and left singular vectors of the
 * n_signals x (n_trials n_tapers) coefficient matrix per (window, two-sided bin) are the leading
 * eigenpairs of the cross-spectral matrix; parallel cyclic Jacobi in LDS, n_signals <=
 * sc_global_coherence_max_signals() (256; beyond 64 signals the eigenvectors come from a logged rotation
 * sequence applied to batches of unit vectors, any max_rank <= n_signals, and the call synchronises the stream).  d_accum: records with SC_PLANE_CSM accumulated over
 * trials and tapers, N or N/2+1 bins per window (real-input symmetry completes the rest).
 * d_values: double [n_groups][N][max_rank]; d_vectors: complex128 [n_groups][N][n_signals][max_rank],
 * unit norm, largest component real positive (the reference's phase is LAPACK's/ARPACK's).
 * ascending != 0 orders the max_rank largest values smallest-first (scipy svds, which the reference
 * takes when max_rank < n_signals - 1). */
int sc_global_coherence_max_signals(void);
int sc_global_coherence_f64(const void* d_accum, int64_t n_groups, int64_t n_freq_accum, int64_t N,
                            int64_t n_signals, uint32_t planes, int64_t n_observations, int max_rank,
                            int ascending, double* d_values, void* d_vectors /*complex128*/, void* stream);

/* ---- canonical coherence between channel groups (fp64, from the accumulated CSM) -------
 * Replaces Connectivity.canonical_coherence, _normalize_fourier_coefficients and
 * _estimate_canonical_coherence (connectivity.py:745-820, :1979-2032): per (bin, group pair)
 * the squared largest singular value of L_g^-1 S_gh L_h^-H with S_gg = L_g L_g^H.
 *   d_members   int32 [n_groups][stride] channel indices of every group, stride = 16 if
 *               max_group_size <= 16, 32 if <= 32, else 128 (max supported: sc_canonical_max_group() = 128)
 *   d_sizes     int32 [n_groups]
 *   d_out       double [n_bins][n_groups][n_groups], symmetric, NaN diagonal
 *   d_fail      int32 [1]: number of (bin, group pair) items with a group block that was not positive definite (their
 *               entries of d_out are NaN; a bad group counts once for every pair it is in)
 * Groups of <= 16 channels take a stream-ordered workspace of n_bins * n_groups * 4 KB for the
 * inverted group factors, groups beyond 64 channels one of 768 KB per persistent workgroup (<= 256) for the blocks of
 * the pair in flight (hipMallocAsync / hipFreeAsync on `stream`); SC_ENOMEM if that fails.  17 ... 64 channels: a
 * persistent workgroup per (bin, group pair) item with the whole problem in LDS (round 6), no workspace. */
int sc_canonical_max_group(void);
int sc_canonical_coherence_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                               int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                               int n_groups, int max_group_size, double* d_out, int32_t* d_fail,
                               void* stream);

/* ---- multivariate imaginary coherence between channel groups (fp64, from the accumulated CSM) ----
 * The leakage-robust group measures of Ewald, Marzetti, Zappasodi, Meinecke & Nolte 2012 (NeuroImage 62:1964-1971), per
 * (bin, group pair), with R_g = Re S_gg, I = Im S_ab and D = R_a^-1/2 I R_b^-1/2:
 *     MIC = sigma_max(D)                                 in [0, 1]
 *     MIM = sum_k sigma_k(D)^2 = tr(R_a^-1 I R_b^-1 I^T)   in [0, min(n_a, n_b)]
 * Both are 0 wherever the cross-spectrum is real.  The kernels and conventions of sc_canonical_coherence_f64 (same member
 * table and stride, group sizes up to sc_canonical_max_group(), workspace, argument checks and error codes) on a second read
 * view of the records -- group blocks (Re S, 0), cross blocks (0, Im S) -- always with the Householder / Sturm kernels.
 *   d_mic, d_mim  double [n_bins][n_groups][n_groups], symmetric, NaN diagonal
 *   d_fail        int32 [1]: number of pairs with a group block whose real part was not positive definite (NaN in both) */
int sc_imaginary_interaction_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                 int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                 int n_groups, int max_group_size, double* d_mic, double* d_mim,
                                 int32_t* d_fail, void* stream);

/* ---- the vectors that attain MIC (fp64; sc_canonical.hip; additive, ABI v8) ----
 * Per (bin, group pair a < b), with R_g = L_g L_g^T, M = L_a^-1 I L_b^-T, p the unit eigenvector of M M^T for MIC^2 and
 * q = M^T p / MIC:   filters  alpha = L_a^-T p, beta = L_b^-T q   (alpha^T R_a alpha = beta^T R_b beta = 1, alpha^T I beta = MIC)
 *                    patterns a = L_a p = R_a alpha, b = L_b q = R_b beta   (I beta = MIC a, I^T alpha = MIC b).
 * One joint sign per pair: the entry of pattern a with the largest magnitude (lowest index on a tie) is positive.
 * Arguments, member table, checks and error codes of sc_imaginary_interaction_f64.
 *   d_mic                  double [n_bins][n_groups][n_groups], symmetric, NaN diagonal
 *   d_filters, d_patterns  double [n_bins][n_groups][n_groups][max_group_size]: entry [a][b][0 .. n_a) is group a's vector in
 *                          its interaction with group b (both orders of a pair are filled), NaN beyond n_a, on the diagonal,
 *                          for a pair whose MIC is NaN and for a pair whose M is exactly 0 (MIC 0: no direction is singled out)
 *   d_fail                 int32 [1]: as sc_imaginary_interaction_f64
 * One 256-thread workgroup per (bin, pair), persistent; parallel Jacobi on M M^T with a rotation log.  A pair whose groups
 * have at most sc_interaction_vectors_lds_group(max_group_size) channels keeps its three blocks in LDS, the others in a
 * stream-ordered scratch of 768 KB per workgroup; the rotation log takes 14 (n - 1) (n / 2) 24 bytes per workgroup
 * (n = max_group_size rounded up to even: 2.7 MB at 128 channels; 256 ... 1024 workgroups), from the same allocation
 * (hipMallocAsync / hipFreeAsync on `stream`, SC_ENOMEM if that fails). */
int sc_interaction_vectors_lds_group(int max_group_size);
int sc_imaginary_interaction_vectors_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                         int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                         int n_groups, int max_group_size, double* d_mic, double* d_filters,
                                         double* d_patterns, int32_t* d_fail, void* stream);

/* ---- the vectors that attain canonical coherence, and its whole spectrum (fp64; sc_canonical.hip; additive, ABI v8) ----
 * Per (bin, group pair a < b) of the records as sc_canonical_coherence_f64 reads them, with S_gg = L_g L_g^H, M = L_a^-1 S_ab L_b^-H,
 * rho_1 >= rho_2 >= ... the singular values of M (the canonical coherences; sc_canonical_coherence_f64 gives rho_1^2), p the unit
 * eigenvector of M M^H for rho_1^2 and q = M^H p / rho_1:
 *     filters  alpha = L_a^-H p, beta = L_b^-H q   (alpha^H S_aa alpha = beta^H S_bb beta = 1, alpha^H S_ab beta = rho_1, real)
 *     patterns a = L_a p = S_aa alpha, b = L_b q = S_bb beta   (S_ab beta = rho_1 a, S_ab^H alpha = rho_1 b).
 * One joint unit phase per pair: the entry of pattern a with the largest magnitude (lowest index on a tie) is real and positive.
 * Arguments, member table, checks and error codes of sc_imaginary_interaction_vectors_f64.
 *   d_coherence            double [n_bins][n_groups][n_groups]: rho_1, symmetric, NaN diagonal
 *   d_coherences           double [n_bins][n_groups][n_groups][max_group_size]: rho_k = sqrt(clamp(lambda_k, 0, 1)), descending,
 *                          the same in [a][b] and [b][a]; NaN beyond min(n_a, n_b), on the diagonal and for a failed pair
 *   d_filters, d_patterns  double [n_bins][n_groups][n_groups][max_group_size][2] (re, im): entry [a][b][0 .. n_a) is group a's
 *                          vector in its pairing with group b (both orders of a pair are filled), NaN beyond n_a, on the diagonal,
 *                          for a failed pair and for a pair whose M is exactly 0 (every rho_k 0: no direction is singled out)
 *   d_fail                 int32 [1]: number of pairs with a group block that was not positive definite (NaN in every output)
 * One 256-thread workgroup per (bin, pair), persistent; parallel Jacobi on the packed Hermitian M M^H with a rotation log.  A pair
 * whose groups have at most sc_canonical_vectors_lds_group(max_group_size) channels keeps its three blocks in LDS, the others in
 * a stream-ordered scratch; workspace as sc_imaginary_interaction_vectors_f64. */
int sc_canonical_vectors_lds_group(int max_group_size);
int sc_canonical_coherence_vectors_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                       int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                       int n_groups, int max_group_size, double* d_coherence, double* d_coherences,
                                       double* d_filters, double* d_patterns, int32_t* d_fail, void* stream);

/* ---- partial and multiple coherence (fp64, from the accumulated CSM; sc_partial.hip; additive, ABI v8) ----
 * The coherence of two signals after the linear influence of all the other signals is removed, and the share of a signal's
 * power that all the others explain linearly (the reference has neither).  Per bin record, with S the normalised Hermitian
 * n_signals x n_signals cross-spectral matrix and G = S^-1:
 *     partial coherency              gamma_ij = -G_ij / sqrt(G_ii G_jj)     Hermitian; two signals: S_01 / sqrt(S_00 S_11)
 *     partial coherence magnitude    |gamma_ij|                             in [0, 1], not squared
 *     multiple coherence magnitude   R_i = sqrt(max(0, 1 - 1 / (S_ii G_ii)))   in [0, 1)
 * All three are unchanged under S -> D S D (D a positive diagonal); the kernel inverts the unit-diagonal D^-1/2 S D^-1/2, D = diag S,
 * by a Cholesky factorisation, one 256-thread workgroup per record with the whole problem in LDS (17 C^2 / 2 bytes and a
 * few rows: 136 KB at 128 signals) -- no workspace.  2 <= n_signals <= sc_partial_coherence_max_signals() = 128.
 *   d_accum       records with SC_PLANE_CSM, n_bins of them (as sc_canonical_coherence_f64; same checks and error codes,
 *                 SC_EINVAL also for n_signals outside the range and for three NULL outputs)
 *   d_coherency   complex128 [n_bins][n_signals][n_signals] or NULL, NaN diagonal
 *   d_magnitude   double [n_bins][n_signals][n_signals] or NULL, symmetric, NaN diagonal
 *   d_multiple    double [n_bins][n_signals] or NULL
 *   d_fail        int32 [1]: number of records without an inverse -- a channel without (finite) power, or a Cholesky pivot of
 *                 the scaled matrix that is not finite or <= n_signals 2^-52; NaN in all of their outputs */
int sc_partial_coherence_max_signals(void);
int sc_partial_coherence_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                             int64_t n_observations, void* d_coherency /*complex128*/, double* d_magnitude,
                             double* d_multiple, int32_t* d_fail, void* stream);

/* ---- partial and multiple coherence given a chosen set of signals (sc_partial.hip; additive, ABI v8) ----
 * The same measures with a chosen conditioning set (FieldTrip's partchannel): the coherence of the kept signals after the m
 * given signals Z -- and only those -- are regressed out of each, and the share of a kept signal's power that the given ones
 * explain.  Per bin record, with A the a kept signals (disjoint from Z) and the residual cross-spectrum
 *     E = S_AA - S_AZ S_ZZ^-1 S_ZA = S_AA - W^H W,   W = L^-1 S_ZA,   S_ZZ = L L^H:
 *     partial coherency given Z      gamma_ij = E_ij / sqrt(E_ii E_jj)          Hermitian, i, j in A
 *     magnitude                      |gamma_ij|                                 in [0, 1], not squared
 *     multiple coherence given Z     R_i = sqrt(max(0, 1 - E_ii / S_ii))        in [0, 1]
 * All three are unchanged under S -> D S D; the kernel works on the unit-diagonal S', where r_i = E'_ii = 1 - sum_k |W_ki|^2 and
 * R_i = sqrt(sum_k |W_ki|^2).  One 256-thread workgroup per record, no workspace; resident in LDS are the packed triangle of Z,
 * W [m][a] and three rows of doubles:
 *     sc_partial_given_lds_bytes(a, m) = (m (m + 1) / 2 + m a) * 16 + (2 a + m) * 8 + 16   (-1 outside the two ranges below)
 * which must not exceed sc_partial_given_lds_limit() = 160 KB: 1024 kept given 8 (145 KB), 512 given 16 (138 KB), 300 given 6
 * (33 KB), 14 given 128 (158 KB), and every a + m <= 128.  1 <= m <= sc_partial_given_max_given() = 128,
 * 1 <= a <= sc_partial_given_max_kept() = 1024, a + m <= n_signals.
 *   d_accum       records as for sc_partial_coherence_f64 (same checks and error codes; SC_EINVAL also for sizes outside the
 *                 limits and for three NULL outputs; SC_EHIP if the device refuses the dynamic LDS)
 *   d_kept        int32 [n_kept], d_given int32 [n_given]: device arrays of distinct signal indices in [0, n_signals); the
 *                 outputs are in the order of d_kept.  An index outside the range fails its problems (its record is not read).
 *   d_coherency   complex128 [n_bins][a][a] or NULL, NaN diagonal
 *   d_magnitude   double [n_bins][a][a] or NULL, symmetric, NaN diagonal
 *   d_multiple    double [n_bins][a] or NULL
 *   d_fail        int32 [2]: [0] records that failed -- a kept or given signal without (finite) power, or a Cholesky pivot of
 *                 the scaled Z block that is not finite or <= m 2^-52 (two identical given signals) --, NaN in all of their
 *                 outputs; [1] (record, kept signal) cases with r_i <= (m + 1) 2^-52 or not finite -- the given signals explain
 *                 the signal entirely (a copy of one of them): NaN in its row and column, R_i = 1, nothing else affected */
int     sc_partial_given_max_given(void);
int     sc_partial_given_max_kept(void);
int64_t sc_partial_given_lds_bytes(int64_t n_kept, int64_t n_given);
int64_t sc_partial_given_lds_limit(void);
int sc_partial_coherence_given_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                   int64_t n_observations, const int32_t* d_kept, int n_kept, const int32_t* d_given,
                                   int n_given, void* d_coherency /*complex128 [n_bins][a][a]*/, double* d_magnitude,
                                   double* d_multiple /*[n_bins][a]*/, int32_t* d_fail /*[2]*/, void* stream);

/* ---- total, instantaneous and lagged linear dependence (fp64; sc_dependence.hip; additive, ABI v8) ----
 * Pascual-Marqui's decomposition of the linear dependence between two groups of signals (arXiv:0706.1776; Phil. Trans. R. Soc. A
 * 369:3768, 2011; "lagged coherence" of LORETA-KEY and FieldTrip; the reference has none of it).  Per (bin, pair of disjoint
 * groups a, b with p and q signals, J = a then b), S the normalised Hermitian cross-spectral matrix:
 *     F_total         = ln det S_aa    + ln det S_bb    - ln det S_JJ        = -sum_k ln(1 - rho_k^2), rho_k the canonical coherences
 *     F_instantaneous = ln det Re S_aa + ln det Re S_bb - ln det Re S_JJ
 *     F_lagged        = F_total - F_instantaneous                            0 wherever the cross-spectrum is real
 * (Pascual-Marqui's coherences are 1 - exp(-F).)  All three are symmetric in (a, b) and unchanged under S -> D S D; the kernels
 * work on the unit-diagonal matrix.  Arguments, member table and stride, checks and error codes of sc_imaginary_interaction_f64.
 *   d_total, d_instantaneous, d_lagged   double [n_bins][n_groups][n_groups], symmetric, NaN diagonal; any may be NULL, not all
 *                 three (SC_EINVAL)
 *   d_fail        int32 [1]: the (bin, pair) problems that failed, NaN in every output -- a member without finite positive power
 *                 (or outside the record), or a pivot of one of the unit-diagonal Cholesky factorisations that is not finite or
 *                 <= n 2^-52 (n = p + q, for the block of b alone n = q)
 * A pair with p + q > n_observations has a singular joint matrix: it is left NaN, not computed and not counted.  A pair with
 * p + q > sc_linear_dependence_max_joint() = 128 gives SC_EUNSUPPORTED before any kernel is launched, the message naming the
 * size: from max_group_size alone where that decides (a group of 128 has no partner), else -- only when two groups of
 * max_group_size would exceed the limit -- from the two largest entries of d_sizes, which are then read back first (one small
 * copy and a wait on `stream`).
 * max_group_size = 1 (every group a single signal; any n_signals): one thread per entry, closed forms of the coherency c,
 *     -log1p(-|c|^2), -log1p(-(Re c)^2), log1p((Im c)^2 / (1 - |c|^2)); NaN and counted where 1 - |c|^2 <= 0.  No workspace.
 * Groups: a 256-thread persistent workgroup per (bin, pair) factorises the packed lower triangle of S'_JJ in LDS (132 KB at
 * n = 128), then of Re S'_JJ with a real-typed routine on half the bytes; 2 sum_{k >= p} ln L_kk of each is ln det (JJ) -
 * ln det (aa).  The determinants of the b blocks come from a first launch per (bin, group) that fills a [n_bins][n_groups][2]
 * table in a stream-ordered workspace (hipMallocAsync / hipFreeAsync on `stream`; SC_ENOMEM if that fails). */
int sc_linear_dependence_max_joint(void);
int sc_linear_dependence_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                             int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                             int n_groups, int max_group_size, double* d_total, double* d_instantaneous,
                             double* d_lagged, int32_t* d_fail, void* stream);

/* ---- delete-one jackknife of power and coherence (sc_jackknife.hip; additive, ABI v8) ------------------------
 * Standard errors that rest on the data (Thomson & Chave 1991; Chronux coherencyc / mtspectrumc with err = [2 p]); the
 * reference has only the closed forms of statistics.py.  Per kept index and bin the delete units u = 1 .. n hold g
 * observations each, G_u = sum over the unit's observations of x_i conj(x_j), S = sum_u G_u is the un-normalised CSM record
 * (SC_PLANE_CSM of sc_csm_accumulate_f32 / sc_accumulate_f64 ..., summed over every rank's trials), and for each measure
 *     d_u = theta(S - G_u) - theta(S),
 *     SC_JACKKNIFE_POWER                theta = ln(S_ii / n_observations_used)              [n_bins][C]
 *     SC_JACKKNIFE_COHERENCE_MAGNITUDE  theta = atanh(|S_ij| / sqrt(S_ii S_jj))             [n_bins][C][C], diagonal NaN
 *     SC_JACKKNIFE_IMAGINARY_COHERENCE  theta = Im(S_ij) / sqrt(S_ii S_jj), signed          [n_bins][C][C], antisymmetric, diagonal NaN
 * over = SC_JACKKNIFE_OVER_TRIALS: a unit is everything one trial contributes (its reduced windows x tapers; needs
 * desc->reduce_trial); SC_JACKKNIFE_OVER_OBSERVATIONS: every averaged observation is a unit (g = 1).  desc describes the spectra
 * of THIS process (strides, reduce flags; n_freq bins from the first); units [unit_begin, unit_end) of them are walked, and
 * n_units_total >= 2 is the unit count of the whole job (it enters the power statistic).  bin = kept group * n_freq + f as in the
 * records.
 *   d_out   double [sc_jackknife_layout out_doubles]: for each requested measure in the order above three arrays of the shape
 *           given there -- theta(S), sum_u d_u, sum_u d_u^2 over the units walked (partial sums of different processes add).
 *           A channel without power in a bin gives NaN in its entries.  The caller finishes: m = sum d / n,
 *           bias corrected = theta - (n - 1) m, standard error = sqrt((n - 1) / n * (sum d^2 - n m^2)).
 *   d_workspace  sc_jackknife_workspace_bytes (0 when bins x channel tile pairs fill the device; otherwise the units are split
 *           over several workgroups whose partial sums are added in a fixed order).  No floating-point atomics: bit-identical
 *           results from run to run.
 * G_u is summed in the spectra's precision (_f32: complex64 spectra, _f64: complex128); the subtraction, the statistic and the
 * sums are fp64 in both.  d_total: float records, or double with SC_RECORD_F64 in `planes`.  Any n_signals <= 32768 (the kernel
 * tiles the channels itself). */
#define SC_JACKKNIFE_POWER 0x1u
#define SC_JACKKNIFE_COHERENCE_MAGNITUDE 0x2u
#define SC_JACKKNIFE_IMAGINARY_COHERENCE 0x4u
#define SC_JACKKNIFE_OVER_TRIALS 0
#define SC_JACKKNIFE_OVER_OBSERVATIONS 1
int sc_jackknife_layout(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t* n_bins, int64_t* n_units,
                        int64_t* unit_size, int64_t* out_doubles);
int64_t sc_jackknife_workspace_bytes(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t unit_begin,
                                     int64_t unit_end);
int sc_jackknife_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                     uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out,
                     void* d_workspace, int64_t workspace_bytes, void* stream);
int sc_jackknife_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                     uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out,
                     void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- delete-one jackknife of the phase-lag family (sc_jackknife.hip, jk_phase_kernel; additive, ABI v8) -----
 * The same pass, units, `over`, unit range, workspace scheme and output triple (theta, sum_u d_u, sum_u d_u^2) as sc_jackknife_*
 * above, for the measures the reference has no statistics for (FieldTrip: ft_connectivity_wpli's jackknife).  Per observation
 * Im s = Im(x_i conj(x_j)); a unit's sums a_u = sum Im s, b_u = sum |Im s|, c_u = sum sign(Im s), q_u = sum (Im s)^2 (summed in the
 * spectra's precision, c_u an integer) are taken from the totals A, B, N, Q -- the planes SC_PLANE_CSM (im), _ABS_IM, _SIGN_IM and
 * _IM_SQ of d_total -- and with n = n_units_total g observations (n' = (n_units_total - 1) g for a delete-one set), all on the
 * identity scale and in fp64:
 *     SC_JACKKNIFE_PHASE_PLI             theta = N / n                                               antisymmetric
 *     SC_JACKKNIFE_PHASE_WPLI            theta = (A / n) / w, w = B / n, w = 1 where w < 2^-52       antisymmetric
 *     SC_JACKKNIFE_PHASE_DEBIASED_PLI2   theta = (n (N / n)^2 - 1) / (n - 1)                         symmetric
 *     SC_JACKKNIFE_PHASE_DEBIASED_WPLI2  theta = (A^2 - Q) / (B^2 - Q), NaN where B^2 - Q == 0       symmetric
 * (the full estimates are sc_measure_*'s SC_M_PLI, _WPLI, _DEBIASED_PLI2, _DEBIASED_WPLI2 off the diagonal).
 *   d_out   for each requested measure in the order above three double [n_bins][C][C] arrays, diagonal NaN; a NaN d_u makes the
 *           entry's sums NaN.
 *   planes  of d_total; it must hold what the requested measures read: PLI and debiased PLI^2 SC_PLANE_SIGN_IM, wPLI
 *           SC_PLANE_CSM | _ABS_IM, debiased wPLI^2 SC_PLANE_CSM | _ABS_IM | _IM_SQ (float records, or double with SC_RECORD_F64).
 * SC_EINVAL (with sc_last_error) before any launch for: an empty or unknown mask, a bad `over`, a kept trial axis under
 * over = trials, fewer than two units, a unit range outside the spectra, a workspace that is too small, a NULL argument, a
 * missing plane, and a debiased measure whose delete-one sets hold fewer than two observations. */
#define SC_JACKKNIFE_PHASE_PLI 0x1u
#define SC_JACKKNIFE_PHASE_WPLI 0x2u
#define SC_JACKKNIFE_PHASE_DEBIASED_PLI2 0x4u
#define SC_JACKKNIFE_PHASE_DEBIASED_WPLI2 0x8u
int sc_jackknife_phase_layout(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t* n_bins, int64_t* n_units,
                              int64_t* unit_size, int64_t* out_doubles);
int64_t sc_jackknife_phase_workspace_bytes(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t unit_begin,
                                           int64_t unit_end);
int sc_jackknife_phase_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                           uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out,
                           void* d_workspace, int64_t workspace_bytes, void* stream);
int sc_jackknife_phase_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                           uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out,
                           void* d_workspace, int64_t workspace_bytes, void* stream);

/* The total record of sc_jackknife_phase_* from the spectra themselves (jk_phase_totals_kernel): the sums A, B, Q, N over the units
 * [unit_begin, unit_end) of THIS process, as a record of DOUBLES in the accumulator layout with the families `planes` (a non-empty
 * set of SC_PLANE_CSM -- its real plane is 0 --, _ABS_IM, _IM_SQ, _SIGN_IM; hand it on with SC_RECORD_F64 set).  Each total is the
 * fp64 sum of exactly the per-unit sums sc_jackknife_phase_* subtracts from it, whatever the engine: the float32 engine's own
 * records sum thousands of observations in float32, an error in A that the debiased wPLI^2 of a pair with a wPLI near 0 multiplies
 * by B / A (measured: its standard error 6.0e-6 off at 1000 trials), and they take sum Im s and sum |Im s|
 * from different kernels, so that a pair whose Im s never changes sign is not exactly +-1.  Records of different processes add.
 *   d_record     double [n_bins][planes][tiles][16][16] (n_bins and the elements per bin: sc_accum_layout), written whole
 *   d_workspace  sc_jackknife_phase_totals_workspace_bytes (0 unless the units are split over several workgroups)
 * SC_EINVAL before any launch as for sc_jackknife_phase_* (planes instead of measures). */
int64_t sc_jackknife_phase_totals_workspace_bytes(const sc_spectra_desc* desc, uint32_t planes, int over, int64_t unit_begin,
                                                  int64_t unit_end);
int sc_jackknife_phase_totals_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, uint32_t planes, int over,
                                  int64_t unit_begin, int64_t unit_end, double* d_record, void* d_workspace,
                                  int64_t workspace_bytes, void* stream);
int sc_jackknife_phase_totals_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, uint32_t planes, int over,
                                  int64_t unit_begin, int64_t unit_end, double* d_record, void* d_workspace,
                                  int64_t workspace_bytes, void* stream);

/* ---- seed-based connectivity: a few signals against a list of signals (sc_seed.hip; additive, ABI v8) ---------------------
 * What MNE-Connectivity's indices=(seeds, targets) and FieldTrip's channelcmb ask for (the reference has no such call): each of
 * n_seeds signals against each of n_targets signals, for the ten expectation-type measures, in ONE pass over the complex64 /
 * complex128 spectra whatever the measures -- S * C products per observation instead of the C^2 / 2 of the all-pairs records, a
 * record of S * C entries per plane and bin instead of C^2 / 2, no limit of the all-pairs kernels on n_signals.
 *   d_seeds, d_targets  int32 device arrays of signal indices; d_targets == NULL: target t is signal t (n_targets == n_signals).
 *                       The cross-spectrum is s = x_seed conj(x_target).  An index outside [0, n_signals) reads as a signal
 *                       of zeros (no load is issued for it); the hosts refuse such a list before they call.
 *   planes              which sums the record holds: any non-empty set of SC_PLANE_CSM, _ABS_IM, _IM_SQ, _SIGN_IM, _UNIT (as in
 *                       the accumulator records; _UNIT is the product of the unit phasors x / |x| of the two factors), and
 *                       SC_SEED_PLANE_POWER for sum |x_seed|^2, sum |x_target|^2 (what the coherency family divides by).
 *   d_record            double [n_bins][planes in accumulator order][n_seeds][n_targets], then with SC_SEED_PLANE_POWER
 *                       double [n_seeds], double [n_targets] per bin: sc_seed_record_layout doubles per bin, n_bins = kept
 *                       groups x desc->n_freq as in sc_accum_layout.  Un-normalised sums, fp64 on both engines (products in the
 *                       spectra's precision): the records of trial shards add.  Written whole.
 *   d_workspace         sc_seed_accumulate_workspace_bytes, 16-byte aligned (0 where bins x target tiles x seed chunks fill the
 *                       device; otherwise the observations are split over several workgroups whose partial records are added
 *                       in split order: no floating-point atomics, bit-identical from run to run)
 * sc_seed_measure_f64: record -> measures, SC_M_COHERENCY (complex), _COHERENCE_MAGNITUDE, _COHERENCE_PHASE,
 * _IMAGINARY_COHERENCE (these four need SC_PLANE_CSM | SC_SEED_PLANE_POWER), SC_M_PLV, _PPC (SC_PLANE_UNIT), SC_M_PLI,
 * _DEBIASED_PLI2 (_SIGN_IM), SC_M_WPLI (_CSM | _ABS_IM), SC_M_DEBIASED_WPLI2 (_CSM | _ABS_IM | _IM_SQ): d_outs[m] is
 * [n_bins][n_seeds][n_targets] of double / double2 (wide[m] != 0) or float / float2, with the algebra of sc_measure_* entry for
 * entry, n_observations the count of the whole job; where seed s IS target t the value is what that measure has on its diagonal.
 * SC_EINVAL before any launch for a NULL pointer, n_seeds outside 1 ... sc_seed_connectivity_max_seeds(), n_targets outside
 * 1 ... 32768, planes outside the set above (or SC_SEED_PLANE_POWER alone), a measure that is not one of the ten or whose planes
 * the record lacks, and a workspace smaller than the query's answer. */
#define SC_SEED_PLANE_POWER 0x20u
int sc_seed_connectivity_max_seeds(void);
int sc_seed_record_layout(int64_t n_seeds, int64_t n_targets, uint32_t planes, int64_t* doubles_per_bin);
int64_t sc_seed_accumulate_workspace_bytes(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t planes);
int sc_seed_accumulate_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                           const int32_t* d_targets, int64_t n_targets, uint32_t planes, double* d_record, void* d_workspace,
                           int64_t workspace_bytes, void* stream);
int sc_seed_accumulate_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                           const int32_t* d_targets, int64_t n_targets, uint32_t planes, double* d_record, void* d_workspace,
                           int64_t workspace_bytes, void* stream);
int sc_seed_measure_f64(const double* d_record, int64_t n_bins, const int32_t* d_seeds, int64_t n_seeds, const int32_t* d_targets,
                        int64_t n_targets, uint32_t planes, int64_t n_observations, int n_measures, const int* measures,
                        const int* wide, void* const* d_outs, void* stream);

/* ---- delete-one jackknife of seed-based connectivity (sc_seed_jackknife.hip; additive, ABI v8) ------------------------------
 * The statistic of sc_jackknife_* and sc_jackknife_phase_* above -- units, `over`, unit range, d_u = theta(total - unit) -
 * theta(total), the output triple (theta, sum_u d_u, sum_u d_u^2) -- for each of n_seeds signals against each of n_targets
 * signals, with d_seeds, d_targets, the index rules and s = x_seed conj(x_target) of sc_seed_accumulate_*: n_seeds x n_targets
 * entries per unit instead of C^2 / 2, no [n_bins][C][C] array.  One mask covers both families, on the scales given there:
 *     SC_SEED_JACKKNIFE_COHERENCE_MAGNITUDE  theta = atanh(|S| / sqrt(P_seed P_target))           reads SC_PLANE_CSM | SC_SEED_PLANE_POWER
 *     SC_SEED_JACKKNIFE_IMAGINARY_COHERENCE  theta = Im S / sqrt(P_seed P_target), signed         reads SC_PLANE_CSM | SC_SEED_PLANE_POWER
 *     SC_SEED_JACKKNIFE_PLI                  theta = N / n                                        reads SC_PLANE_SIGN_IM
 *     SC_SEED_JACKKNIFE_WPLI                 theta = (A / n) / w, w = B / n, 1 where w < 2^-52    reads SC_PLANE_CSM | _ABS_IM
 *     SC_SEED_JACKKNIFE_DEBIASED_PLI2        theta = (n (N / n)^2 - 1) / (n - 1)                  reads SC_PLANE_SIGN_IM
 *     SC_SEED_JACKKNIFE_DEBIASED_WPLI2       theta = (A^2 - Q) / (B^2 - Q), NaN where B^2 - Q == 0   reads SC_PLANE_CSM | _ABS_IM | _IM_SQ
 * with S = sum s, A = Im S, B = sum |Im s|, N = sum sign(Im s), Q = sum (Im s)^2, P = sum |x|^2 and n = n_units_total g
 * observations (n' = (n_units_total - 1) g in a delete-one set).  Unit sums are taken in the spectra's precision (the sign count
 * is an integer); the subtraction, the statistic and the sums are fp64 on both engines.  The sums of d are taken about the first
 * unit's deviation of a workgroup and moved back, so an entry whose units all have the same deviation has sum d^2 = (sum d)^2 / k
 * exactly.  Where seed s IS target t the three outputs are NaN; a NaN d_u makes the entry's sums NaN; a signal without power
 * gives NaN in the coherency pair.
 *
 * sc_seed_jackknife_totals_*: the totals from the spectra themselves, as a seed record of doubles (sc_seed_record_layout) with
 * `planes` = a set of SC_PLANE_CSM, _ABS_IM, _IM_SQ, _SIGN_IM with at least one of them, and SC_SEED_PLANE_POWER (SC_PLANE_UNIT
 * is refused): the same walk and the same unit sums as sc_seed_jackknife_*, added over the units [unit_begin, unit_end) in fp64,
 * so a total is the sum of exactly the unit sums that are subtracted from it.  Written whole; records of trial shards add;
 * sc_seed_measure_f64 reads it like any seed record.
 *   d_total      such a record, summed over every rank's units; `planes` must hold what the requested measures read
 *   d_out        double [sc_seed_jackknife_layout out_doubles]: for each requested measure in the order above three
 *                double [n_bins][n_seeds][n_targets] arrays -- theta, sum_u d_u, sum_u d_u^2 over the units walked (partial
 *                sums of different processes add; theta is the same in all of them)
 *   d_workspace  sc_seed_jackknife_workspace_bytes / sc_seed_jackknife_totals_workspace_bytes, 16-byte aligned (0 where bins x
 *                target tiles x seed chunks fill the device; otherwise the units are split over up to 256 workgroups of at least
 *                16 units whose partial sums are added in split order: no floating-point atomics, bit-identical from run to run)
 * SC_EINVAL (with sc_last_error) before any launch for everything sc_jackknife_phase_* and sc_seed_accumulate_* refuse -- a NULL
 * argument, bad counts, an empty or unknown mask or plane set, a bad `over`, a kept trial axis under over = trials, fewer than two
 * units, a unit range outside the spectra, a debiased measure whose delete-one sets hold fewer than two observations, a workspace
 * that is too small or misaligned -- and for a total record that lacks a plane a requested measure reads. */
#define SC_SEED_JACKKNIFE_COHERENCE_MAGNITUDE 0x1u
#define SC_SEED_JACKKNIFE_IMAGINARY_COHERENCE 0x2u
#define SC_SEED_JACKKNIFE_PLI 0x4u
#define SC_SEED_JACKKNIFE_WPLI 0x8u
#define SC_SEED_JACKKNIFE_DEBIASED_PLI2 0x10u
#define SC_SEED_JACKKNIFE_DEBIASED_WPLI2 0x20u
int sc_seed_jackknife_layout(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t measures, int over,
                             int64_t* n_bins, int64_t* n_units, int64_t* unit_size, int64_t* out_doubles);
int64_t sc_seed_jackknife_workspace_bytes(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t measures,
                                          int over, int64_t unit_begin, int64_t unit_end);
int64_t sc_seed_jackknife_totals_workspace_bytes(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t planes,
                                                 int over, int64_t unit_begin, int64_t unit_end);
int sc_seed_jackknife_totals_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                 const int32_t* d_targets, int64_t n_targets, uint32_t planes, int over, int64_t unit_begin,
                                 int64_t unit_end, double* d_record, void* d_workspace, int64_t workspace_bytes, void* stream);
int sc_seed_jackknife_totals_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                 const int32_t* d_targets, int64_t n_targets, uint32_t planes, int over, int64_t unit_begin,
                                 int64_t unit_end, double* d_record, void* d_workspace, int64_t workspace_bytes, void* stream);
int sc_seed_jackknife_f32(const void* d_X /*float2*/, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                          const int32_t* d_targets, int64_t n_targets, const double* d_total, uint32_t planes, uint32_t measures,
                          int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out, void* d_workspace,
                          int64_t workspace_bytes, void* stream);
int sc_seed_jackknife_f64(const void* d_X /*double2*/, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                          const int32_t* d_targets, int64_t n_targets, const double* d_total, uint32_t planes, uint32_t measures,
                          int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out, void* d_workspace,
                          int64_t workspace_bytes, void* stream);

/* ---- host-pointer side of the boundary: memory, copies, streams (sc_memory.hip, ABI v3) ---------------------
 * What the reference's CuPy backend does with `xp.asarray(time_series)` on the way in and `.get()` on the way out
 * (transforms.py:405-439, connectivity.py:31-65): with these a host that has only ctypes + NumPy drives the whole path
 * (spectral_connectivity_amd/numpy_host.py); a PyTorch host may keep its own allocator -- every compute entry point
 * takes raw device pointers from either.
 *   sc_device_alloc / sc_device_free   stream-ordered pool allocation (hipMallocAsync / hipFreeAsync on `stream`)
 *   sc_host_alloc / sc_host_free       page-locked host memory (copies at link rate, asynchronous on their stream)
 *   sc_host_register / _unregister     pin a buffer the host already owns (a NumPy array) for the same effect
 *   sc_memcpy_h2d / sc_memcpy_d2h      asynchronous on `stream` for page-locked host memory; from / to pageable memory
 *                                      the runtime stages the copy and returns when the host buffer is reusable
 *   sc_memset_zero, sc_stream_create (non-blocking), sc_stream_destroy, sc_stream_synchronize
 * sc_nonfinite_f32 / _f64: the constructor's NaN / infinity scan of the time series (transforms.py:746-753) on the
 * device: *d_flag |= 1 if any of the n samples is not finite (caller zeroes the flag, reads it after a sync). */
int sc_device_alloc(void** d_ptr, size_t bytes, void* stream);
int sc_device_free(void* d_ptr, void* stream);
int sc_host_alloc(void** h_ptr, size_t bytes);
int sc_host_free(void* h_ptr);
int sc_host_register(void* h_ptr, size_t bytes);
int sc_host_unregister(void* h_ptr);
int sc_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
int sc_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
int sc_memset_zero(void* d_ptr, size_t bytes, void* stream);
int sc_stream_create(void** stream);
int sc_stream_destroy(void* stream);
int sc_stream_synchronize(void* stream);
int sc_nonfinite_f32(const float* d_x, int64_t n, int32_t* d_flag, void* stream);
int sc_nonfinite_f64(const double* d_x, int64_t n, int32_t* d_flag, void* stream);

/* ---- amplitude range of the float32 engine -----------------------------------------------------------------------------------
 * The float32 stage-B kernels square products of coefficients: (Im s)^2 is of the order |x|^4, which leaves the float32 range for
 * coefficients of 1e-13 (MEG in tesla), and no float32 record can hold such a sum.  A host asks for the size of the coefficients
 * before it sends such a request to the float32 kernels and accumulates a float64 record from a complex128 copy otherwise
 * (spectral_connectivity_amd/_stage_abc.py: amplitude_guard, with the thresholds).
 *   sc_amplitude_range_f32   dense complex64 rows [n_rows][C] -> d_out double[2][C]: sum |x_c|^2, max(|Re x_c|, |Im x_c|); partial
 *                            sums folded in a fixed order (the same bits on every run); d_work: sc_amplitude_range_work_bytes
 *   sc_spectra_widen_f32     n complex64 numbers -> complex128 (exact) */
int64_t sc_amplitude_range_work_bytes(int64_t n_rows, int64_t C);
int sc_amplitude_range_f32(const void* d_X /*float2*/, int64_t n_rows, int64_t C, double* d_out, void* d_work, int64_t work_bytes,
                           void* stream);
int sc_spectra_widen_f32(const void* d_X /*float2*/, int64_t n, void* d_out /*double2*/, void* stream);

/* ---- Exchange of trial-sharded records over RCCL / xGMI (SURVEY section 8(b) `sc_allreduce`, 8(e)) ------------------------
 * The reference has no multi-device path (its CuPy backend is one GPU: transforms.py:405-439, connectivity.py:31-65); trials
 * shard over one process per GPU because the expectation is a plain sum of per-observation terms (connectivity.py:67-75,
 * :489): every rank accumulates its trials into un-normalised records, the records are summed, sc_measure_* normalises by the
 * TOTAL observation count.  These calls are that sum for a host without torch.distributed (the PyTorch host's form of the same
 * steps is parallel.py; SC_EXCHANGE=library routes it through here):
 *   sc_comm_unique_id            128 bytes from ONE rank, carried to the others by the host (file, socket, MPI, torch ...)
 *   sc_comm_create               one communicator per process on the current device (ncclCommInitRank)
 *   sc_comm_exchange_blocks_f32  block j of d_send -> rank j, d_recv[i] <- rank i: all N - 1 links at once (the direct reduce-
 *                                scatter; sc_measure_multi_parts sums the received blocks in rank order while it reads them)
 *   sc_comm_allreduce_f32        in-place sum of a whole record buffer (ring form)
 *   sc_comm_gather_f32           n floats of every rank -> d_recv[rank][n] on root
 * RCCL is bound at run time (dlopen librccl.so.1): without it sc_comm_available() is 0 and the calls return SC_EUNSUPPORTED. */
typedef struct sc_comm sc_comm;
int sc_comm_available(void);
int sc_comm_unique_id(void* id128);
int sc_comm_create(const void* id128, int n_ranks, int rank, sc_comm** out);
int sc_comm_destroy(sc_comm* comm);
int sc_comm_size(const sc_comm* comm, int* n_ranks, int* rank);
int sc_comm_allreduce_f32(sc_comm* comm, float* d_buf, int64_t n, void* stream);
int sc_comm_exchange_blocks_f32(sc_comm* comm, const float* d_send, float* d_recv, int64_t block, void* stream);
int sc_comm_gather_f32(sc_comm* comm, const float* d_send, float* d_recv, int64_t n, int root, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SC_HIP_H */
