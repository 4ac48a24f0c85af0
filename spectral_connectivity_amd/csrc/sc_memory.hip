// sc_memory.hip -- the host-pointer side of the boundary (ownership row): device and page-locked
// host memory, copies and streams as plain C calls, so that a host with nothing but ctypes + NumPy can drive the
// engine (spectral_connectivity_amd/numpy_host.py, tests/test_abi.py) -- the reference's `xp.asarray(...)` upload and
// `.get()` download of its CuPy backend (transforms.py:405-439, connectivity.py:31-65).  PyTorch hosts keep using
// their own allocator and streams: every compute entry point takes raw device pointers from either.
#include "sc_common.h"

// d_out[0 .. n) = NaN on the stream: the "not computed" default of the stage-D outputs
__global__ void fill_nan_kernel(double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = nan("");
}
void sc_internal_fill_nan(double* d_out, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(fill_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_out, n);
}

// The default pool hands freed memory back to the driver at the next synchronisation (release threshold 0): every
// allocation of a steady-state loop would then be a real hipMalloc.  Keep what was freed (one setting per device).
static void keep_pool_memory() {
    static bool done[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || done[dev]) return;
    done[dev] = true;
    hipMemPool_t pool = nullptr;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
        uint64_t keep = UINT64_MAX;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    (void)hipGetLastError();
}

extern "C" int sc_device_alloc(void** d_ptr, size_t bytes, void* stream) {
    SC_REQUIRE(d_ptr != nullptr, "NULL argument");
    *d_ptr = nullptr;
    if (bytes == 0) return SC_OK;
    keep_pool_memory();
    // stream-ordered pool allocation: a freed block is handed out again without a trip to the driver
    hipError_t e = hipMallocAsync(d_ptr, bytes, (hipStream_t)stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sc_set_error("sc_device_alloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        *d_ptr = nullptr;
        return e == hipErrorOutOfMemory ? SC_ENOMEM : SC_EHIP;
    }
    return SC_OK;
}

extern "C" int sc_device_free(void* d_ptr, void* stream) {
    if (!d_ptr) return SC_OK;
    SC_CHECK_HIP(hipFreeAsync(d_ptr, (hipStream_t)stream));
    return SC_OK;
}

extern "C" int sc_host_alloc(void** h_ptr, size_t bytes) {
    SC_REQUIRE(h_ptr != nullptr, "NULL argument");
    *h_ptr = nullptr;
    if (bytes == 0) return SC_OK;
    hipError_t e = hipHostMalloc(h_ptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sc_set_error("sc_host_alloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        *h_ptr = nullptr;
        return SC_ENOMEM;
    }
    return SC_OK;
}

extern "C" int sc_host_free(void* h_ptr) {
    if (!h_ptr) return SC_OK;
    SC_CHECK_HIP(hipHostFree(h_ptr));
    return SC_OK;
}

// Pinning a buffer the host already owns (a NumPy array): the copy engines then read / write it directly, no staging
// copy through the runtime's own bounce buffers.
extern "C" int sc_host_register(void* h_ptr, size_t bytes) {
    SC_REQUIRE(h_ptr != nullptr && bytes > 0, "NULL argument");
    SC_CHECK_HIP(hipHostRegister(h_ptr, bytes, hipHostRegisterDefault));
    return SC_OK;
}
extern "C" int sc_host_unregister(void* h_ptr) {
    SC_REQUIRE(h_ptr != nullptr, "NULL argument");
    SC_CHECK_HIP(hipHostUnregister(h_ptr));
    return SC_OK;
}

extern "C" int sc_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    if (bytes == 0) return SC_OK;
    SC_REQUIRE(d_dst != nullptr && h_src != nullptr, "NULL argument");
    SC_CHECK_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return SC_OK;
}

extern "C" int sc_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream) {
    if (bytes == 0) return SC_OK;
    SC_REQUIRE(h_dst != nullptr && d_src != nullptr, "NULL argument");
    SC_CHECK_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SC_OK;
}

extern "C" int sc_memset_zero(void* d_ptr, size_t bytes, void* stream) {
    if (bytes == 0) return SC_OK;
    SC_REQUIRE(d_ptr != nullptr, "NULL argument");
    SC_CHECK_HIP(hipMemsetAsync(d_ptr, 0, bytes, (hipStream_t)stream));
    return SC_OK;
}

extern "C" int sc_stream_create(void** stream) {
    SC_REQUIRE(stream != nullptr, "NULL argument");
    hipStream_t s = nullptr;
    SC_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return SC_OK;
}
extern "C" int sc_stream_destroy(void* stream) {
    if (!stream) return SC_OK;
    SC_CHECK_HIP(hipStreamDestroy((hipStream_t)stream));
    return SC_OK;
}
extern "C" int sc_stream_synchronize(void* stream) {
    SC_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return SC_OK;
}

// ---- device-side finite check -----------------------------------------------------------------------------------
// The reference scans the time series on the host in its constructor (transforms.py:746-753: a warning when any sample
// is NaN or infinite).  On the device the same scan is one read of the uploaded series at HBM rate: every thread ORs
// the exponent-all-ones test of its samples, one atomicOr per workgroup that saw one.
template <typename T>
__global__ void __launch_bounds__(256) nonfinite_kernel(const T* __restrict__ x, int64_t n, int32_t* flag) {
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const T v = x[i];
        bad |= !(fabs((double)v) <= 1.7976931348623157e308);      // false for NaN and for +-inf
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
__global__ void __launch_bounds__(256) nonfinite4_kernel(const float4* __restrict__ x, int64_t n4, int32_t* flag) {
    unsigned bad = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 v = x[i];
        // exponent field all ones <=> NaN or infinity
        bad |= ((__float_as_uint(v.x) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(v.y) & 0x7f800000u) == 0x7f800000u) |
               ((__float_as_uint(v.z) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(v.w) & 0x7f800000u) == 0x7f800000u);
    }
    if (__any((int)bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// *d_flag |= 1 when any of the n samples is NaN or +-inf (the caller zeroes the flag; reads it after the stream drains)
extern "C" int sc_nonfinite_f32(const float* d_x, int64_t n, int32_t* d_flag, void* stream) {
    SC_REQUIRE(d_flag != nullptr && (d_x != nullptr || n == 0) && n >= 0, "NULL argument");
    if (n == 0) return SC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n4 = (((uintptr_t)d_x) % 16 == 0) ? n / 4 : 0;
    if (n4) {
        const int grid = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
        hipLaunchKernelGGL(nonfinite4_kernel, dim3(grid), dim3(256), 0, s, (const float4*)d_x, n4, d_flag);
    }
    if (n - 4 * n4) hipLaunchKernelGGL(nonfinite_kernel<float>, dim3(1), dim3(256), 0, s, d_x + 4 * n4, n - 4 * n4, d_flag);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}
extern "C" int sc_nonfinite_f64(const double* d_x, int64_t n, int32_t* d_flag, void* stream) {
    SC_REQUIRE(d_flag != nullptr && (d_x != nullptr || n == 0) && n >= 0, "NULL argument");
    if (n == 0) return SC_OK;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(nonfinite_kernel<double>, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_x, n, d_flag);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}

// ---- amplitude range of complex64 spectra and their complex128 copy: the float32 engine's guard (_stage_abc.amplitude_guard) ------
// A float32 record cannot hold sums of (Im s)^2 ~ |x|^4 for coefficients of 1e-13 (MEG in tesla).  Before a request that squares
// products runs on the float32 kernels, the host asks for the per-channel size of the coefficients: d_out[0][c] = sum |x_c|^2 (in
// double: the squares themselves leave the float32 range) and d_out[1][c] = max(|Re x_c|, |Im x_c|) over dense rows [n_rows][C].
// Two launches, partial sums per row slice folded in slice order: the same bits on every run (the statistic picks the engine).
#define SC_AMP_PARTS_MAX 1024

static int amp_parts(int64_t n_rows) {
    const int64_t want = (n_rows + 3) / 4;
    return (int)(want < 1 ? 1 : want > SC_AMP_PARTS_MAX ? SC_AMP_PARTS_MAX : want);
}

__global__ void __launch_bounds__(256) amplitude_part_kernel(const float2* __restrict__ X, int64_t n_rows, int C,
                                                             double* __restrict__ part /*[gridDim.y][2][C]*/) {
    __shared__ double s_sq[4][64];
    __shared__ float s_mx[4][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    double sq = 0.0;
    float mx = 0.f;
    if (c < C)
        for (int64_t r = (int64_t)blockIdx.y * 4 + ry; r < n_rows; r += (int64_t)gridDim.y * 4) {
            const float2 v = X[r * C + c];
            sq += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
            mx = fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y)));
        }
    s_sq[ry][cx] = sq;
    s_mx[ry][cx] = mx;
    __syncthreads();
    if (ry == 0 && c < C) {
        part[((int64_t)blockIdx.y * 2 + 0) * C + c] = (s_sq[0][cx] + s_sq[1][cx]) + (s_sq[2][cx] + s_sq[3][cx]);
        part[((int64_t)blockIdx.y * 2 + 1) * C + c] = (double)fmaxf(fmaxf(s_mx[0][cx], s_mx[1][cx]), fmaxf(s_mx[2][cx], s_mx[3][cx]));
    }
}

__global__ void amplitude_fold_kernel(const double* __restrict__ part, int n_parts, int C, double* __restrict__ out /*[2][C]*/) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sq = 0.0, mx = 0.0;
    for (int k = 0; k < n_parts; ++k) {
        sq += part[((int64_t)k * 2 + 0) * C + c];
        mx = fmax(mx, part[((int64_t)k * 2 + 1) * C + c]);
    }
    out[c] = sq;
    out[C + c] = mx;
}

extern "C" int64_t sc_amplitude_range_work_bytes(int64_t n_rows, int64_t C) {
    if (n_rows < 1 || C < 1) return 0;
    return (int64_t)amp_parts(n_rows) * 2 * C * (int64_t)sizeof(double);
}

extern "C" int sc_amplitude_range_f32(const void* d_X, int64_t n_rows, int64_t C, double* d_out, void* d_work, int64_t work_bytes,
                                      void* stream) {
    SC_REQUIRE(d_X && d_out && d_work, "NULL argument");
    SC_REQUIRE(n_rows >= 1 && C >= 1 && C <= (1 << 20), "empty or oversized dimension");
    SC_REQUIRE(work_bytes >= sc_amplitude_range_work_bytes(n_rows, C), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int parts = amp_parts(n_rows);
    hipLaunchKernelGGL(amplitude_part_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)parts), dim3(256), 0, s, (const float2*)d_X,
                       n_rows, (int)C, (double*)d_work);
    hipLaunchKernelGGL(amplitude_fold_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const double*)d_work, parts, (int)C,
                       d_out);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}

// d_out[i] = (double) d_X[i], i < n complex numbers: the complex128 copy of complex64 spectra (exact)
__global__ void widen_kernel(const float2* __restrict__ X, int64_t n, double2* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float2 v = X[i];
        out[i] = make_double2((double)v.x, (double)v.y);
    }
}

extern "C" int sc_spectra_widen_f32(const void* d_X, int64_t n, void* d_out, void* stream) {
    SC_REQUIRE(d_X && d_out && n >= 1, "NULL argument or empty spectra");
    const int grid = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(widen_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float2*)d_X, n, (double2*)d_out);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}
