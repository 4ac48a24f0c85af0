// sc_wilson_loop.h -- the host side of the batched Wilson iteration, shared by the 2 x 2 form (sc_wilson.hip) and the C x C
// form (sc_mvar.hip): the rocFFT pair of the lengths the one-kernel causal projection (sc_wilson_fft.hip) does not take, the
// convergence flags, and the queue-then-poll loop.  The stream is synchronised once per WILSON_POLL iterations: every
// iteration logs how many problems are still running into its own slot, converged problems are skipped by every kernel, so
// queueing a few iterations past the last convergence changes nothing but costs empty launches.
#pragma once
#include <rocfft/rocfft.h>
#include "sc_common.h"

#define WILSON_HIST 1024     // iterations whose "still running" counts the workspace can log (max_iterations <= this)
#define WILSON_POLL 4        // iterations queued between two looks at the counts
// (group, pair) problems of the 2 x 2 form: gridDim.y holds at most 65535 of them, gridDim.z the rest
#define WILSON_PMAX 65535

#define SC_CHECK_FFT(expr)                                                                       \
    do {                                                                                         \
        rocfft_status s_ = (expr);                                                               \
        if (s_ != rocfft_status_success) {                                                       \
            sc_set_error("%s failed: rocfft_status %d (%s:%d)", #expr, (int)s_, __FILE__, __LINE__); \
            return SC_EFFT;                                                                      \
        }                                                                                        \
    } while (0)

__device__ inline void atomic_max_nonneg(double* addr, double v) {
    // order of non-negative doubles == order of their bit patterns
    atomicMax(reinterpret_cast<unsigned long long*>(addr), (unsigned long long)__double_as_longlong(v));
}

// status: 0 running -> 1 converged (err < tol); counts iterations; clears err; *n_running = #still 0 (one slot per
// iteration: the host reads the slots of a whole batch of iterations at once)
static __global__ void wilson_flags(int32_t* status, int32_t* n_iter, double* err, double tol, int64_t P, int32_t* n_running) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    if (status[p] == 0) {
        n_iter[p] += 1;
        if (err[p] < tol) status[p] = 1;
        else atomicAdd(n_running, 1);
    }
    err[p] = 0.0;
}

// after the (unnormalised) inverse FFT of the C x C series A[p][e][n]: 1/N, halve lag 0, zero the strict lower triangle at
// lag 0, zero the non-causal half (minimum_phase_decomposition.py:96-142).  PAIRS: the grid of the 2 x 2 form (problems over
// blockIdx.y and .z, a thread walks the entries), else problems in blockIdx.z and the entries over blockIdx.y.
template <bool PAIRS>
static __global__ void wilson_causal(double2* A, int64_t N, int C, int64_t P) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = PAIRS ? (int64_t)blockIdx.z * WILSON_PMAX + blockIdx.y : (int64_t)blockIdx.z;
    if (n >= N || p >= P) return;
    for (int e = PAIRS ? 0 : blockIdx.y; e < C * C; e += PAIRS ? 1 : gridDim.y) {
        const int i = e / C, j = e % C;
        double sc = (n < (N + 1) / 2) ? 1.0 / (double)N : 0.0;
        if (n == 0) { sc *= 0.5; if (i > j) sc = 0.0; }
        double2* a = A + (p * C * C + e) * N + n;
        *a = make_double2(a->x * sc, a->y * sc);
    }
}

// The in-place complex128 transforms of `batch` series of length N (cached plans: sc_internal_z2z_plan), their work buffer
// and execution info.  Constructed by every call, init() only where the one-kernel projection does not apply.
struct WilsonFft {
    rocfft_plan fwd = nullptr, inv = nullptr;
    bool fwd_cached = false, inv_cached = false;
    rocfft_execution_info info = nullptr;
    void* work = nullptr;
    hipStream_t st = nullptr;
    WilsonFft() {
        static int rocfft_ready = 0;
        if (!rocfft_ready) { rocfft_setup(); rocfft_ready = 1; }
    }
    WilsonFft(const WilsonFft&) = delete;
    WilsonFft& operator=(const WilsonFft&) = delete;
    ~WilsonFft() {
        if (info) rocfft_execution_info_destroy(info);
        if (fwd && !fwd_cached) rocfft_plan_destroy(fwd);       // (cached plans live as long as the process: sc_internal_z2z_plan)
        if (inv && !inv_cached) rocfft_plan_destroy(inv);
        if (work) (void)hipFreeAsync(work, st);
    }
    int init(size_t N, size_t batch, hipStream_t stream) {
        int rc;
        size_t ws_f = 0, ws_i = 0;
        st = stream;
        if ((rc = sc_internal_z2z_plan(&fwd, 1, N, batch, &fwd_cached)) != SC_OK) return rc;
        if ((rc = sc_internal_z2z_plan(&inv, 0, N, batch, &inv_cached)) != SC_OK) return rc;
        SC_CHECK_FFT(rocfft_plan_get_work_buffer_size(fwd, &ws_f));
        SC_CHECK_FFT(rocfft_plan_get_work_buffer_size(inv, &ws_i));
        SC_CHECK_FFT(rocfft_execution_info_create(&info));
        if (ws_f < ws_i) ws_f = ws_i;
        if (ws_f) {
            if (hipMallocAsync(&work, ws_f, st) != hipSuccess) { sc_set_error("rocFFT work buffer alloc failed"); return SC_ENOMEM; }
            SC_CHECK_FFT(rocfft_execution_info_set_work_buffer(info, work, ws_f));
        }
        SC_CHECK_FFT(rocfft_execution_info_set_stream(info, st));
        return SC_OK;
    }
    // A <- fft(causal(ifft(A))) on the series A[p][e][n], e < C * C; `grid`: the caller's launch grid of wilson_causal<PAIRS>
    template <bool PAIRS>
    int causal(void* A, int64_t N, int C, int64_t P, dim3 grid) {
        void* bufs[1] = {A};
        SC_CHECK_FFT(rocfft_execute(inv, bufs, nullptr, info));
        hipLaunchKernelGGL(wilson_causal<PAIRS>, grid, dim3(256), 0, st, (double2*)A, N, C, P);
        SC_CHECK_FFT(rocfft_execute(fwd, bufs, nullptr, info));
        return SC_OK;
    }
};

// The counters of one run in the caller's workspace: err [P]; n_fallback, `fallback_bytes` in all, with the WILSON_HIST
// slots of the "still running" counts behind it.
struct WilsonCounters {
    double* err;
    int32_t* n_iter;         // [P] (the caller's output)
    int32_t* status;         // [P]
    int32_t* n_fallback;
    size_t fallback_bytes;
    int32_t* n_running() const { return (int32_t*)((char*)n_fallback + fallback_bytes); }
};
struct WilsonLoopResult { int iters, running, rc; };

// Clears the counters, has `start()` queue the launches that put the initial factor in place, then queues `step()` (one
// iteration, up to its error reduction into c.err; both return an SC_ code) and the flags kernel WILSON_POLL times between two
// looks at the slots, until no problem runs or max_iter.
template <class Start, class Step>
static WilsonLoopResult wilson_loop(const WilsonCounters& c, int64_t P, double tol, int max_iter, hipStream_t st, Start start,
                                    Step step) {
    WilsonLoopResult r = {0, (int)P, SC_OK};
    int queued = 0;
    int32_t hist[WILSON_POLL];
    if (max_iter > WILSON_HIST) {
        sc_set_error("max_iterations = %d exceeds the %d iterations the workspace can log", max_iter, WILSON_HIST);
        r.rc = SC_EINVAL;
        return r;
    }
    (void)hipMemsetAsync(c.err, 0, (size_t)P * 8, st);
    (void)hipMemsetAsync(c.n_iter, 0, (size_t)P * 4, st);
    (void)hipMemsetAsync(c.n_fallback, 0, c.fallback_bytes + (size_t)WILSON_HIST * 4, st);      // fallback count + the slots
    if ((r.rc = start()) != SC_OK) return r;
    while (queued < max_iter && r.running > 0) {
        const int first = queued;
        for (int b = 0; b < WILSON_POLL && queued < max_iter; ++b, ++queued) {
            if ((r.rc = step()) != SC_OK) return r;
            hipLaunchKernelGGL(wilson_flags, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, c.status, c.n_iter, c.err, tol, P,
                               c.n_running() + queued);
        }
        if (hipMemcpyAsync(hist, c.n_running() + first, (size_t)(queued - first) * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            sc_set_error("Wilson iterations %d..%d: %s", first, queued, hipGetErrorString(hipGetLastError()));
            r.rc = SC_EHIP;
            return r;
        }
        for (int b = 0; b < queued - first; ++b) {
            r.running = hist[b];
            r.iters = first + b + 1;
            if (r.running == 0) break;
        }
    }
    return r;
}
