// sc_partial.hip -- partial and multiple coherence from the accumulated cross-spectral records (fp64, up to 128 signals).
//
// Per problem (one bin record) with S the normalised Hermitian C x C cross-spectral matrix and G = S^-1:
//     partial coherency    gamma_ij = -G_ij / sqrt(G_ii G_jj)               (C = 2: the ordinary coherency S_01 / sqrt(S_00 S_11))
//     multiple coherence   R_i      = sqrt(max(0, 1 - 1 / (S_ii G_ii)))
// Both are unchanged under S -> D S D for a positive diagonal D, so the kernel works on S' = D^-1/2 S D^-1/2 with D = diag S:
// the unit diagonal makes the pivot test below a statement about the condition number, whatever the channels' units, and
// S'_ii G'_ii = G'_ii.
//
// One 256-thread workgroup per problem, the whole problem in dynamic LDS (no global scratch, no atomics but the fail counter):
//     P     [C (C + 1) / 2] complex   packed lower triangle, row i at i (i + 1) / 2: S', then its Cholesky factor L, then M = L^-1
//     row   [C]             complex   the row of L that the inversion is replacing
//     dg    [C]             double    S_ii
//     gd    [C]             double    G'_jj
//     flag  [4]             int       the problem failed
// 17 C^2 / 2 + ... bytes: 136 208 B at C = 128 (one workgroup a compute unit), 35 344 B at C = 64 (four), 2 704 B at C = 16.
// Steps: load and scale; right-looking Cholesky on the packed layout (a pivot that is not finite or <= C 2^-52 fails the
// problem); M = L^-1 in place, row by row from the top -- row i of L goes to `row`, then M_ij = -(1 / L_ii) sum_{k=j}^{i-1}
// row[k] M_kj reads only rows of M that are final; G'_jj = sum_{k>=j} |M_kj|^2; one (i >= j) pair per thread and step,
// G'_ij = sum_{k>=i} conj(M_ki) M_kj, written at (i, j) and mirrored at (j, i).  A failed problem is NaN in every output.
#include "sc_common.h"

namespace {

typedef double2 cd;
constexpr int PC_MAX_C = 128;
constexpr int PC_THREADS = 256;
// Ablation for tools/partial_coherence_time.py --steps: a library built with -DPC_STEPS=n ends every problem after step n of the
// list above (1 load, 2 Cholesky, 3 inverse, 4 diagonal; results wrong by design).  The shipped library runs all five.
#ifndef PC_STEPS
#define PC_STEPS 5
#endif

struct PartialArgs {
    ScRec accum;
    ScCsmView v;
    int C;
    int64_t n_bins;
    cd* coherency;       // [n_bins][C][C] or NULL
    double* magnitude;   // [n_bins][C][C] or NULL
    double* multiple;    // [n_bins][C] or NULL
    int32_t* fail;
};

__host__ __device__ constexpr size_t pc_lds_bytes(int C) {
    return ((size_t)C * (C + 1) / 2 + C) * sizeof(cd) + (size_t)2 * C * sizeof(double) + 16;
}

__device__ __forceinline__ int pc_row(int i) { return i * (i + 1) / 2; }

// (i, j), j <= i, of the packed index t < 8256 + 128: float sqrt, corrected to the exact row
__device__ __forceinline__ void pc_unpack(int t, int& i, int& j) {
    int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (pc_row(r + 1) <= t) ++r;
    while (pc_row(r) > t) --r;
    i = r; j = t - pc_row(r);
}

// In-place lower Cholesky of the n x n Hermitian matrix in the packed lower triangle P (row i at i (i + 1) / 2), all 256 threads,
// right-looking like sc_wg_cholesky.  A pivot that is not finite or not above `floor` sets *bad and ends the factorisation: every
// thread reads the same pivot, so all of them leave at the same k.  Two barriers a column: every thread takes the square root
// itself, and thread 0 stores it only after the column is scaled (nobody reads the diagonal entry again).  The trailing triangle
// goes to 16 groups of 16 lanes, a group walking rows and its lanes the columns of a row -- no index arithmetic per entry beyond
// one row offset --, two entries a lane with their loads ahead of the first store (the compiler cannot move a load of P above a
// store to P).
__device__ inline void pc_cholesky_packed(cd* P, int n, double floor, int* bad) {
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    for (int k = 0; k < n; ++k) {
        const double d = P[pc_row(k) + k].x;
        if (!(d > floor) || !isfinite(d)) {
            if (tid == 0) *bad = 1;
            break;
        }
        const double dk = sqrt(d), rk = 1.0 / dk;
        for (int i = k + 1 + tid; i < n; i += PC_THREADS) {
            const cd v = P[pc_row(i) + k];
            P[pc_row(i) + k] = make_double2(v.x * rk, v.y * rk);
        }
        __syncthreads();
        if (tid == 0) P[pc_row(k) + k] = make_double2(dk, 0.0);
        for (int i = k + 1 + g; i < n; i += 16) {                    // P[i][j] -= P[i][k] conj(P[j][k]), k < j <= i
            const int ri = pc_row(i);
            const cd a = P[ri + k];
            for (int j = k + 1 + l; j <= i; j += 32) {
                const int j2 = j + 16 <= i ? j + 16 : j;
                const cd b = P[pc_row(j) + k], b2 = P[pc_row(j2) + k], v = P[ri + j], v2 = P[ri + j2];
                P[ri + j] = make_double2(v.x - (a.x * b.x + a.y * b.y), v.y - (a.y * b.x - a.x * b.y));
                if (j2 != j) P[ri + j2] = make_double2(v2.x - (a.x * b2.x + a.y * b2.y), v2.y - (a.y * b2.x - a.x * b2.y));
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PC_THREADS) void partial_coherence_kernel(PartialArgs a) {
    extern __shared__ __attribute__((aligned(16))) char pc_smem[];
    const int C = a.C, tid = threadIdx.x;
    const int n_tri = C * (C + 1) / 2;
    cd* P = reinterpret_cast<cd*>(pc_smem);
    cd* row = P + n_tri;
    double* dg = reinterpret_cast<double*>(row + C);
    double* gd = dg + C;
    int* bad = reinterpret_cast<int*>(gd + C);
    const double qnan = nan("");

    for (int64_t bin = blockIdx.x; bin < a.n_bins; bin += gridDim.x) {
        const ScRec rec = sc_csm_record(a.accum, a.v, 0, bin);
        if (tid == 0) *bad = 0;
        __syncthreads();
        // 1. load and scale to unit diagonal (only the C real channels: the pad channel of an odd count is never read)
        for (int i = tid; i < C; i += PC_THREADS) {
            const double s = sc_csm_entry(rec, a.v, i, i).x;
            const bool ok = s > 0.0 && isfinite(s);
            if (!ok) *bad = 1;
            dg[i] = ok ? s : 1.0;
        }
        __syncthreads();
        for (int e = tid; e < C * C; e += PC_THREADS) {          // i fastest: the records hold the upper triangle, (j, i) row-major
            const int j = e / C, i = e - j * C;
            if (i > j) {
                const cd s = sc_csm_entry(rec, a.v, i, j);
                const double w = sqrt(dg[i] * dg[j]);          // (two identical channels: exactly 1, and an exactly zero pivot)
                P[pc_row(i) + j] = make_double2(s.x / w, s.y / w);
            } else if (i == j) {
                P[pc_row(i) + i] = make_double2(1.0, 0.0);
            }
        }
        __syncthreads();
        // 2. Cholesky S' = L L^H
        if (PC_STEPS >= 2 && !*bad) pc_cholesky_packed(P, C, (double)C * 0x1p-52, bad);
        __syncthreads();
        const bool failed = *bad != 0;
        if (!failed && PC_STEPS >= 3) {
            // 3. M = L^-1 in place, top to bottom; a thread pair per column j shares the sum over k
            for (int i = 0; i < C; ++i) {
                for (int k = tid; k <= i; k += PC_THREADS) row[k] = P[pc_row(i) + k];
                __syncthreads();
                const double ri = 1.0 / row[i].x;
                const int j = tid >> 1, half = tid & 1;
                if (j < i) {
                    double sx = 0.0, sy = 0.0;
                    int k = i - 1 - half;
                    for (; k - 6 >= j; k -= 8) {                    // four terms with their loads together
                        cd l[4], m[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) { l[u] = row[k - 2 * u]; m[u] = P[pc_row(k - 2 * u) + j]; }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            sx += l[u].x * m[u].x - l[u].y * m[u].y;
                            sy += l[u].x * m[u].y + l[u].y * m[u].x;
                        }
                    }
                    for (; k >= j; k -= 2) {
                        const cd l = row[k], m = P[pc_row(k) + j];
                        sx += l.x * m.x - l.y * m.y;
                        sy += l.x * m.y + l.y * m.x;
                    }
                    sx += __shfl_xor(sx, 1);
                    sy += __shfl_xor(sy, 1);
                    if (half == 0) P[pc_row(i) + j] = make_double2(-ri * sx, -ri * sy);
                } else if (tid == 2 * i) {
                    P[pc_row(i) + i] = make_double2(ri, 0.0);
                }
                __syncthreads();
            }
            // 4. G'_jj = sum_{k >= j} |M_kj|^2
            if (PC_STEPS >= 4) {
                const int j = tid >> 1, half = tid & 1;
                double s = 0.0;
                if (j < C)
                    for (int k = j + half; k < C; k += 2) {
                        const cd m = P[pc_row(k) + j];
                        s += m.x * m.x + m.y * m.y;
                    }
                s += __shfl_xor(s, 1);
                if (j < C && half == 0) gd[j] = s;
            }
            __syncthreads();
        }
        // 5. outputs (6.: NaN everywhere for a failed problem)
        cd* oc = a.coherency ? a.coherency + bin * C * C : nullptr;
        double* om = a.magnitude ? a.magnitude + bin * C * C : nullptr;
        for (int t = tid; t < (PC_STEPS >= 5 ? n_tri : 0); t += PC_THREADS) {
            int i, j;
            pc_unpack(t, i, j);
            double gx = qnan, gy = qnan;
            if (!failed && i != j) {
                double sx = 0.0, sy = 0.0;                         // conj(M_ki) M_kj
                int k = i;
                for (; k + 3 < C; k += 4) {
                    cd p[4], q[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { p[u] = P[pc_row(k + u) + i]; q[u] = P[pc_row(k + u) + j]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        sx += p[u].x * q[u].x + p[u].y * q[u].y;
                        sy += p[u].x * q[u].y - p[u].y * q[u].x;
                    }
                }
                for (; k < C; ++k) {
                    const cd p = P[pc_row(k) + i], q = P[pc_row(k) + j];
                    sx += p.x * q.x + p.y * q.y;
                    sy += p.x * q.y - p.y * q.x;
                }
                const double w = -1.0 / sqrt(gd[i] * gd[j]);
                gx = sx * w; gy = sy * w;
            }
            if (oc) {
                oc[i * C + j] = make_double2(gx, gy);
                if (i != j) oc[j * C + i] = make_double2(gx, -gy);
            }
            if (om) {
                const double mag = i == j ? qnan : sqrt(gx * gx + gy * gy);
                om[i * C + j] = mag;
                if (i != j) om[j * C + i] = mag;
            }
        }
        if (a.multiple)
            for (int i = tid; i < C; i += PC_THREADS) {
                const double r = 1.0 - 1.0 / gd[i];
                a.multiple[bin * C + i] = failed ? qnan : sqrt(r > 0.0 ? r : 0.0);
            }
        if (failed && tid == 0) atomicAdd(a.fail, 1);
        __syncthreads();                                           // (the next problem overwrites P, gd and the flag)
    }
}

}  // namespace

extern "C" int sc_partial_coherence_max_signals(void) { return PC_MAX_C; }

extern "C" int sc_partial_coherence_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                        int64_t n_observations, void* d_coherency, double* d_magnitude, double* d_multiple,
                                        int32_t* d_fail, void* stream) {
    ScTimed timed_("partial_coherence", stream);
    SC_REQUIRE(d_accum && d_fail, "NULL argument");
    SC_REQUIRE(d_coherency || d_magnitude || d_multiple, "no output requested");
    PartialArgs a;
    const int rcv = sc_csm_view(planes, n_bins, n_bins, n_signals, n_observations, &a.v);
    if (rcv != SC_OK) return rcv;
    SC_REQUIRE(n_bins >= 1, "empty problem");
    SC_REQUIRE(n_signals >= 2, "partial coherence needs at least two signals");
    if (n_signals > PC_MAX_C) {
        sc_set_error("invalid argument: partial coherence supports at most %d signals (got %lld)", PC_MAX_C, (long long)n_signals);
        return SC_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    a.accum = sc_rec(d_accum, planes); a.C = (int)n_signals; a.n_bins = n_bins;
    a.coherency = static_cast<cd*>(d_coherency); a.magnitude = d_magnitude; a.multiple = d_multiple; a.fail = d_fail;
    // every LDS index of the kernel is a function of C alone, and 2 <= C <= PC_MAX_C here
    const size_t lds = pc_lds_bytes(a.C);
    static_assert(pc_lds_bytes(PC_MAX_C) <= 160 * 1024, "the largest problem must fit LDS");
    SC_CHECK_HIP(hipMemsetAsync(d_fail, 0, 4, st));
    SC_CHECK_HIP(hipFuncSetAttribute((const void*)partial_coherence_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // persistent workgroups: as many a compute unit as their LDS allows (at most 8: 2048 threads)
    int per_cu = (int)((160 * 1024) / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int64_t want = (int64_t)256 * per_cu;
    const unsigned blocks = (unsigned)(n_bins < want ? n_bins : want);
    hipLaunchKernelGGL(partial_coherence_kernel, dim3(blocks), dim3(PC_THREADS), lds, st, a);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}
