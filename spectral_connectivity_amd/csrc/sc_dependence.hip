// sc_dependence.hip -- total, instantaneous and lagged linear dependence between signals or groups of signals (Pascual-Marqui
// 2007, arXiv:0706.1776; Pascual-Marqui et al. 2011, Phil. Trans. R. Soc. A 369:3768), fp64, from the accumulated cross-spectral
// records.
//
// Per (bin record, pair of disjoint groups a, b with p and q signals; J = a then b), S the normalised Hermitian matrix:
//     F_total         = ln det S_aa    + ln det S_bb    - ln det S_JJ
//     F_instantaneous = ln det Re S_aa + ln det Re S_bb - ln det Re S_JJ
//     F_lagged        = F_total - F_instantaneous
// All three are unchanged under S -> D S D for a positive diagonal D, so everything below works on the unit-diagonal S' (as
// sc_partial.hip does): the pivot floor n 2^-52 is then a statement about the condition number, whatever the channels' units.
//
// Tier 1, every group a single signal (dep_pairwise_kernel): no factorisation; one thread per entry of a 16 x 16 tile, with
// c = S'_ij:   F_total = -log1p(-|c|^2),   F_inst = -log1p(-(Re c)^2),   F_lagged = log1p((Im c)^2 / (1 - |c|^2))
// -- exactly 0 for a real cross-spectrum.  1 - |c|^2 <= 0 or a signal without (finite) power: NaN, counted.
//
// Tier 2, groups (p + q <= 128): 256-thread persistent workgroups, one problem at a time in dynamic LDS
//     P     [n (n + 1) / 2] complex   packed lower triangle (row i at i (i + 1) / 2) of S'_JJ, then its Cholesky factor; afterwards
//                                     the same bytes hold the REAL packed triangle of Re S'_JJ (half of them) and its factor
//     dg    [n]             double    S_ii of the members
//     idx   [n]             int       the members' signal indices, a then b
//     red   [4] double, flag [4] int
// 16 n (n + 1) / 2 + 12 n + 48 bytes: 133 680 B at n = 128 (one workgroup a compute unit), 34 096 B at n = 64 (four, the most the
// registers admit).
// Because the leading p x p block of L_JJ is L_aa, ln det S_JJ - ln det S_aa = 2 sum_{k >= p} ln L_kk: ONE factorisation of the
// joint matrix gives two of the three terms, and a second one of its real part (a real-typed instance of the same routine on half
// the bytes -- no zeros through the complex one) the same two of the instantaneous part.  ln det S'_bb and ln det Re S'_bb come
// from a first launch of the same routine per (bin, group) with the split at 0 (dep_group_kernel), which writes a
// [n_bins][n_groups][2] table into a stream-ordered allocation; the pair kernel (dep_pair_kernel) reads its group b entry.
// A problem fails (NaN in every output, counted once) when a member has no finite positive power, lies outside the record, or a
// pivot of one of the factorisations -- the pair's two or group b's two -- is not finite or <= n 2^-52.
#include <stdlib.h>
#include "sc_common.h"

namespace {

typedef double2 cd;
constexpr int LD_MAX_JOINT = 128;
constexpr int LD_THREADS = 256;
constexpr size_t LD_LDS_LIMIT = 160 * 1024;

struct DepArgs {
    ScRec accum;
    ScCsmView v;
    const int32_t* members;   // [G][mstride]
    const int32_t* sizes;     // [G]
    int G, mstride, n_signals, lds_n, grp_n;   // lds_n / grp_n: the largest pair / group the launch reserved LDS for
    int64_t n_bins, n_obs;
    double* total;            // [n_bins][G][G] or NULL
    double* inst;
    double* lagged;
    int32_t* fail;
};

__host__ __device__ constexpr size_t ld_lds_bytes(int n) {
    return (size_t)n * (n + 1) / 2 * sizeof(cd) + (size_t)n * sizeof(double) + (((size_t)n * sizeof(int) + 15) & ~(size_t)15) +
           4 * sizeof(double) + 16;
}

__device__ __forceinline__ int ld_row(int i) { return i * (i + 1) / 2; }

// the two element types of the factorisation: v - a conj(b), r v, the real part and the embedding of a real
__device__ __forceinline__ cd ld_msub(cd v, cd a, cd b) {
    return make_double2(v.x - (a.x * b.x + a.y * b.y), v.y - (a.y * b.x - a.x * b.y));
}
__device__ __forceinline__ double ld_msub(double v, double a, double b) { return v - a * b; }
__device__ __forceinline__ cd ld_scale(cd v, double r) { return make_double2(v.x * r, v.y * r); }
__device__ __forceinline__ double ld_scale(double v, double r) { return v * r; }
__device__ __forceinline__ double ld_re(cd v) { return v.x; }
__device__ __forceinline__ double ld_re(double v) { return v; }
__device__ __forceinline__ void ld_set(cd* p, double x) { *p = make_double2(x, 0.0); }
__device__ __forceinline__ void ld_set(double* p, double x) { *p = x; }

// In-place lower Cholesky of the n x n Hermitian (T = cd) or symmetric (T = double) matrix in the packed lower triangle P, all 256
// threads, right-looking: pc_cholesky_packed of sc_partial.hip over the element type.  A pivot that is not finite or not above
// `floor` sets *bad and ends the factorisation: every thread reads the same pivot, so all of them leave at the same k.  Two
// barriers a column; the trailing triangle goes to 16 groups of 16 lanes, a group walking rows and its lanes the columns of a
// row, two entries a lane with their loads ahead of the first store.
template <typename T>
__device__ inline void ld_cholesky_packed(T* P, int n, double floor, int* bad) {
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    for (int k = 0; k < n; ++k) {
        const double d = ld_re(P[ld_row(k) + k]);
        if (!(d > floor) || !isfinite(d)) {
            if (tid == 0) *bad = 1;
            break;
        }
        const double dk = sqrt(d), rk = 1.0 / dk;
        for (int i = k + 1 + tid; i < n; i += LD_THREADS) P[ld_row(i) + k] = ld_scale(P[ld_row(i) + k], rk);
        __syncthreads();
        if (tid == 0) ld_set(&P[ld_row(k) + k], dk);
        for (int i = k + 1 + g; i < n; i += 16) {                    // P[i][j] -= P[i][k] conj(P[j][k]), k < j <= i
            const int ri = ld_row(i);
            const T a = P[ri + k];
            for (int j = k + 1 + l; j <= i; j += 32) {
                const int j2 = j + 16 <= i ? j + 16 : j;
                const T b = P[ld_row(j) + k], b2 = P[ld_row(j2) + k], v = P[ri + j], v2 = P[ri + j2];
                P[ri + j] = ld_msub(v, a, b);
                if (j2 != j) P[ri + j2] = ld_msub(v2, a, b2);
            }
        }
        __syncthreads();
    }
}

// 2 sum_{k >= split} ln L_kk of the factor in P (n <= 256: one term a thread); every thread gets the sum
template <typename T>
__device__ inline double ld_log_tail(const T* P, int n, int split, double* red, int tid) {
    const int k = split + tid;
    return 2.0 * sc_wg_sum(k < n ? log(ld_re(P[ld_row(k) + k])) : 0.0, red, tid);
}

__device__ __forceinline__ cd ld_as(cd s, double w, cd*) { return make_double2(s.x / w, s.y / w); }
__device__ __forceinline__ double ld_as(cd s, double w, double*) { return s.x / w; }

// The unit-diagonal S' (T = cd) or Re S' (T = double) of the members idx into the packed triangle P.  Entry e = j n + i, i fastest:
// the records hold the upper triangle, (j, i) row-major.  Four entries a thread and step, their record loads ahead of the first
// store to P (the compiler does not move a load of the record above a store to P).
template <typename T>
__device__ inline void ld_load(const DepArgs& a, ScRec rec, int n, const int* idx, const double* dg, T* P) {
    const cd zero = make_double2(0.0, 0.0);
    for (int e0 = threadIdx.x; e0 < n * n; e0 += 4 * LD_THREADS) {
        cd s[4];
        int i[4], j[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * LD_THREADS;
            j[u] = e / n; i[u] = e - j[u] * n;
            if (e >= n * n) i[u] = -1;                               // (past the end: neither branch below)
            s[u] = i[u] > j[u] ? sc_csm_entry(rec, a.v, idx[i[u]], idx[j[u]]) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i[u] > j[u]) P[ld_row(i[u]) + j[u]] = ld_as(s[u], sqrt(dg[i[u]] * dg[j[u]]), P);
            else if (i[u] == j[u]) ld_set(&P[ld_row(i[u]) + i[u]], 1.0);
        }
    }
}

// The problem whose n member indices the caller has put into idx (and synchronised): *lc = ln det S'_JJ - ln det of its leading
// `split` x `split` block, *lr the same of Re S'.  Returns false (uniformly) for a failed problem.  All 256 threads.
__device__ inline bool ld_log_dets(const DepArgs& a, ScRec rec, int n, int split, char* smem, double* lc, double* lr) {
    const int tid = threadIdx.x;
    cd* P = reinterpret_cast<cd*>(smem);
    double* Pr = reinterpret_cast<double*>(smem);
    double* dg = reinterpret_cast<double*>(P + n * (n + 1) / 2);
    const int* idx = reinterpret_cast<const int*>(dg + n);
    double* red = reinterpret_cast<double*>(smem + ld_lds_bytes(n) - 4 * sizeof(double) - 16);
    int* bad = reinterpret_cast<int*>(red + 4);
    const double floor = (double)n * 0x1p-52;

    if (tid == 0) *bad = 0;
    __syncthreads();
    for (int i = tid; i < n; i += LD_THREADS) {                      // an index outside the record fails the problem unread
        const int c = idx[i];
        bool ok = c >= 0 && c < a.n_signals;
        double s = 1.0;
        if (ok) {
            s = sc_csm_entry(rec, a.v, c, c).x;
            ok = s > 0.0 && isfinite(s);
        }
        if (!ok) *bad = 1;
        dg[i] = ok ? s : 1.0;
    }
    __syncthreads();
    if (*bad) return false;
    __syncthreads();                                                 // (everybody has read the flag before anybody sets it again)
    ld_load<cd>(a, rec, n, idx, dg, P);
    __syncthreads();
    ld_cholesky_packed<cd>(P, n, floor, bad);
    __syncthreads();
    if (*bad) return false;
    *lc = ld_log_tail<cd>(P, n, split, red, tid);                    // (its barriers: nobody reads P or the flag after them)
    ld_load<double>(a, rec, n, idx, dg, Pr);
    __syncthreads();
    ld_cholesky_packed<double>(Pr, n, floor, bad);
    __syncthreads();
    if (*bad) return false;
    *lr = ld_log_tail<double>(Pr, n, split, red, tid);
    return true;
}

__device__ __forceinline__ int* ld_idx(char* smem, int n) {
    return reinterpret_cast<int*>(smem + (size_t)n * (n + 1) / 2 * sizeof(cd) + (size_t)n * sizeof(double));
}

// table[(bin G + g) 2 + {0, 1}] = ln det S'_gg, ln det Re S'_gg; NaN for a group that fails or has more signals than observations
__global__ __launch_bounds__(LD_THREADS) void dep_group_kernel(DepArgs a, double* table, int64_t items) {
    extern __shared__ __attribute__((aligned(16))) char ld_smem[];
    const int tid = threadIdx.x;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t bin = item / a.G;
        const int g = (int)(item - bin * a.G);
        const int n = a.sizes[g];
        double lc = nan(""), lr = nan("");
        if (n >= 1 && n <= a.grp_n && n <= a.mstride && n <= a.n_obs) {
            int* idx = ld_idx(ld_smem, n);
            for (int t = tid; t < n; t += LD_THREADS) idx[t] = a.members[(int64_t)g * a.mstride + t];
            __syncthreads();
            double c = 0.0, r = 0.0;
            if (ld_log_dets(a, sc_csm_record(a.accum, a.v, 0, bin), n, 0, ld_smem, &c, &r)) { lc = c; lr = r; }
        }
        if (tid == 0) { table[item * 2] = lc; table[item * 2 + 1] = lr; }
        __syncthreads();                                             // (the next problem overwrites everything)
    }
}

// one (bin, pair a < b) at a time; the outputs are NaN-filled before the launch
__global__ __launch_bounds__(LD_THREADS) void dep_pair_kernel(DepArgs a, const double* table, int64_t items) {
    extern __shared__ __attribute__((aligned(16))) char ld_smem[];
    const int tid = threadIdx.x;
    const int64_t n_gpairs = (int64_t)a.G * (a.G - 1) / 2;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t bin = item / n_gpairs;
        int ga = 0, rem = (int)(item - bin * n_gpairs);
        while (rem >= a.G - 1 - ga) { rem -= a.G - 1 - ga; ++ga; }
        const int gb = ga + 1 + rem;
        const int na = a.sizes[ga], nb = a.sizes[gb], n = na + nb;
        if (na >= 1 && nb >= 1 && (int64_t)n > a.n_obs) continue;    // a singular joint matrix: left NaN, not counted
        bool ok = na >= 1 && nb >= 1 && n <= a.lds_n && na <= a.mstride && nb <= a.mstride;
        double lc = 0.0, lr = 0.0;
        if (ok) {
            int* idx = ld_idx(ld_smem, n);
            for (int t = tid; t < n; t += LD_THREADS)
                idx[t] = t < na ? a.members[(int64_t)ga * a.mstride + t] : a.members[(int64_t)gb * a.mstride + (t - na)];
            __syncthreads();
            ok = ld_log_dets(a, sc_csm_record(a.accum, a.v, 0, bin), n, na, ld_smem, &lc, &lr);
        }
        if (tid == 0) {
            const double tc = table[(bin * a.G + gb) * 2], tr = table[(bin * a.G + gb) * 2 + 1];
            if (ok && !isnan(tc) && !isnan(tr)) {
                const double ft = tc - lc, fi = tr - lr;
                const int64_t o1 = (bin * a.G + ga) * a.G + gb, o2 = (bin * a.G + gb) * a.G + ga;
                if (a.total) { a.total[o1] = ft; a.total[o2] = ft; }
                if (a.inst) { a.inst[o1] = fi; a.inst[o2] = fi; }
                if (a.lagged) { a.lagged[o1] = ft - fi; a.lagged[o2] = ft - fi; }
            } else {
                atomicAdd(a.fail, 1);
            }
        }
        __syncthreads();                                             // (the next problem overwrites everything)
    }
}

// every group a single signal: entry (ga, gb) of the G x G outputs of one bin per thread, 16 x 16 tiles
__global__ __launch_bounds__(LD_THREADS) void dep_pairwise_kernel(DepArgs a) {
    const int tid = threadIdx.x;
    const int tiles = (a.G + 15) >> 4;
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    const int ga = ti * 16 + (tid >> 4), gb = tj * 16 + (tid & 15);
    const bool in = ga < a.G && gb < a.G;
    const int i = in ? a.members[(int64_t)ga * a.mstride] : -1, j = in ? a.members[(int64_t)gb * a.mstride] : -1;
    const bool valid = in && i >= 0 && i < a.n_signals && j >= 0 && j < a.n_signals;
    const double qnan = nan("");
    for (int64_t bin = blockIdx.y; bin < a.n_bins; bin += gridDim.y) {
        double ft = qnan, fi = qnan, fl = qnan;
        bool failed = false;
        if (in && ga != gb) {
            failed = true;
            if (valid && i != j) {
                const ScRec rec = sc_csm_record(a.accum, a.v, 0, bin);
                const double si = sc_csm_entry(rec, a.v, i, i).x, sj = sc_csm_entry(rec, a.v, j, j).x;
                if (si > 0.0 && isfinite(si) && sj > 0.0 && isfinite(sj)) {
                    const cd s = sc_csm_entry(rec, a.v, i, j);
                    const double w = sqrt(si * sj), re = s.x / w, im = s.y / w;
                    const double re2 = re * re, im2 = im * im, om = 1.0 - (re2 + im2);
                    if (om > 0.0) {                                  // (NaN compares false)
                        ft = -log1p(-(re2 + im2));
                        fi = -log1p(-re2);
                        fl = log1p(im2 / om);
                        failed = false;
                    }
                }
            }
        }
        if (in) {
            const int64_t o = (bin * a.G + ga) * a.G + gb;
            if (a.total) a.total[o] = ft;
            if (a.inst) a.inst[o] = fi;
            if (a.lagged) a.lagged[o] = fl;
        }
        // a failed pair is counted once (ga < gb), one atomic a wave
        const unsigned long long m = __ballot(failed && ga < gb);
        if ((tid & 63) == 0 && m) atomicAdd(a.fail, (int)__popcll(m));
    }
}

}  // namespace

extern "C" int sc_linear_dependence_max_joint(void) { return LD_MAX_JOINT; }

extern "C" int sc_linear_dependence_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                        int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes, int n_groups,
                                        int max_group_size, double* d_total, double* d_instantaneous, double* d_lagged,
                                        int32_t* d_fail, void* stream) {
    ScTimed timed_("linear_dependence", stream);
    SC_REQUIRE(d_accum && d_members && d_sizes && d_fail, "NULL argument");
    SC_REQUIRE(d_total || d_instantaneous || d_lagged, "no output requested");
    DepArgs a;
    const int rcv = sc_csm_view(planes, n_bins, n_bins, n_signals, n_observations, &a.v);
    if (rcv != SC_OK) return rcv;
    SC_REQUIRE(n_groups >= 1 && n_bins >= 1 && n_signals >= 1, "empty problem");
    SC_REQUIRE(max_group_size >= 1, "empty groups");
    SC_REQUIRE(n_signals <= 0x7fffffffLL && n_groups <= 32768 && (double)n_bins * n_groups * n_groups < 4e18, "problem too large");
    // the largest group with any partner: decided by the arguments alone
    if (n_groups >= 2 && max_group_size + 1 > LD_MAX_JOINT) {
        sc_set_error("linear dependence supports pairs of groups with at most %d signals together (a group of %d gives pairs of "
                     "%d or more)", LD_MAX_JOINT, max_group_size, max_group_size + 1);
        return SC_EUNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    a.accum = sc_rec(d_accum, planes); a.members = d_members; a.sizes = d_sizes;
    a.G = n_groups; a.n_signals = (int)n_signals; a.n_bins = n_bins; a.n_obs = n_observations;
    a.mstride = max_group_size <= 16 ? 16 : (max_group_size <= 32 ? 32 : 128);      // (the member table's row length: sc_hip.h)
    a.total = d_total; a.inst = d_instantaneous; a.lagged = d_lagged; a.fail = d_fail;
    a.lds_n = 2 * max_group_size < LD_MAX_JOINT ? 2 * max_group_size : LD_MAX_JOINT;
    if (n_groups >= 2 && 2 * max_group_size > LD_MAX_JOINT) {
        // two groups may exceed the limit together: the two largest sizes decide, read back before any launch
        int32_t* h = (int32_t*)malloc((size_t)n_groups * sizeof(int32_t));
        if (!h) { sc_set_error("linear dependence: out of host memory"); return SC_ENOMEM; }
        hipError_t e = hipMemcpyAsync(h, d_sizes, (size_t)n_groups * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        int big = 0, second = 0;
        for (int g = 0; e == hipSuccess && g < n_groups; ++g) {
            if (h[g] > big) { second = big; big = h[g]; }
            else if (h[g] > second) second = h[g];
        }
        free(h);
        SC_CHECK_HIP(e);
        if (big + second > LD_MAX_JOINT) {
            sc_set_error("linear dependence supports pairs of groups with at most %d signals together (got a pair of %d + %d = %d)",
                         LD_MAX_JOINT, big, second, big + second);
            return SC_EUNSUPPORTED;
        }
        a.lds_n = big + second;
    }
    a.grp_n = max_group_size < a.lds_n ? max_group_size : a.lds_n;
    const int64_t total_out = n_bins * n_groups * n_groups;
    const bool pairwise = max_group_size == 1;
    SC_CHECK_HIP(hipMemsetAsync(d_fail, 0, 4, st));
    if (!pairwise || n_groups < 2) {                                 // (the pairwise kernel writes every entry itself)
        if (d_total) sc_internal_fill_nan(d_total, total_out, st);
        if (d_instantaneous) sc_internal_fill_nan(d_instantaneous, total_out, st);
        if (d_lagged) sc_internal_fill_nan(d_lagged, total_out, st);
    }
    if (n_groups < 2) {
        SC_CHECK_HIP(hipGetLastError());
        return SC_OK;
    }
    if (pairwise) {
        const int64_t tiles = (n_groups + 15) / 16;
        SC_REQUIRE(tiles * tiles <= 0x7fffffffLL, "too many signals");
        const unsigned by = (unsigned)(n_bins < 65535 ? n_bins : 65535);
        hipLaunchKernelGGL(dep_pairwise_kernel, dim3((unsigned)(tiles * tiles), by), dim3(LD_THREADS), 0, st, a);
        SC_CHECK_HIP(hipGetLastError());
        return SC_OK;
    }
    // groups: the block determinants of every (bin, group), then the pairs
    static_assert(ld_lds_bytes(LD_MAX_JOINT) <= LD_LDS_LIMIT, "the largest problem must fit LDS");
    const int64_t g_items = n_bins * n_groups, p_items = n_bins * ((int64_t)n_groups * (n_groups - 1) / 2);
    double* table = nullptr;
    const size_t tbytes = (size_t)g_items * 2 * sizeof(double);
    if (hipMallocAsync((void**)&table, tbytes, st) != hipSuccess) {
        sc_set_error("linear dependence: workspace allocation of %zu bytes failed", tbytes);
        return SC_ENOMEM;
    }
    // every LDS index of the kernels is a function of the problem size n alone, and 1 <= n <= lds_n there
    const size_t lds_g = ld_lds_bytes(a.grp_n), lds_p = ld_lds_bytes(a.lds_n);
    hipError_t rc = hipFuncSetAttribute((const void*)dep_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g);
    if (rc == hipSuccess)
        rc = hipFuncSetAttribute((const void*)dep_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p);
    if (rc == hipSuccess) {
        // Workgroups that walk several problems each: eight shares for every workgroup a compute unit holds at a time (by LDS, at
        // most 4 by registers: profiles/linear_dependence_resource_usage.txt), so that the dispatcher evens out what a grid of
        // exactly the resident count cannot -- a grid beyond it would run its last workgroups alone after all the others.
        int per_cu = (int)(LD_LDS_LIMIT / lds_g);
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
        int64_t want = (int64_t)256 * per_cu * 8;
        hipLaunchKernelGGL(dep_group_kernel, dim3((unsigned)(g_items < want ? g_items : want)), dim3(LD_THREADS), lds_g, st, a, table,
                           g_items);
        per_cu = (int)(LD_LDS_LIMIT / lds_p);
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
        want = (int64_t)256 * per_cu * 8;
        hipLaunchKernelGGL(dep_pair_kernel, dim3((unsigned)(p_items < want ? p_items : want)), dim3(LD_THREADS), lds_p, st, a,
                           (const double*)table, p_items);
    }
    (void)hipFreeAsync(table, st);
    SC_CHECK_HIP(rc);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}
