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

// ---- given a chosen set of signals ----------------------------------------------------------------------------------------
// With Z the m given signals and A the a kept ones, the residual cross-spectrum of A after regressing on Z is
//     E = S_AA - S_AZ S_ZZ^-1 S_ZA = S_AA - W^H W,    W = L^-1 S_ZA,    S_ZZ = L L^H,
// and per (bin, kept pair) gamma_ij = E_ij / sqrt(E_ii E_jj), R_i = sqrt(max(0, 1 - E_ii / S_ii)).  On the unit-diagonal S' as
// above: r_i = E'_ii = 1 - sum_k |W_ki|^2 and R_i = sqrt(sum_k |W_ki|^2).  Only the triangle of Z and W are resident:
//     P     [m (m + 1) / 2] complex   packed lower triangle of S'_ZZ, then its Cholesky factor L
//     W     [m][a]          complex   S'(z_k, a_i), i fastest, then L^-1 of it
//     dg    [m + a]         double    S_ii of the given, then of the kept signals (the latter 1 / sqrt(S_ii) from step 4 on)
//     r     [a]             double    r_i as 1 / sqrt(r_i) (NaN: the kept signal is entirely explained by the given ones)
//     flag  [4]             int       the problem failed
// Steps: diagonal and index check; load both blocks scaled, Cholesky of the Z block (pivot floor m 2^-52); forward elimination
// L W = B, right-looking over the rows of W with one barrier a given signal (row k is scaled by 1 / L_kk one iteration late, when
// nobody reads it any more); r_i and R_i; the pairs, one 8 x 8 tile of (i >= j) pairs a wave and step: the stores at (i, j) and
// their mirrors at (j, i) are then both eight runs of eight neighbours (128 B of coherency each) per wave instruction.
constexpr int PG_MAX_GIVEN = 128;
constexpr int PG_MAX_KEPT = 1024;
constexpr size_t PG_LDS_LIMIT = 160 * 1024;

struct PartialGivenArgs {
    ScRec accum;
    ScCsmView v;
    int a, m, n_signals;
    int64_t n_bins;
    const int32_t* kept;     // [a]
    const int32_t* given;    // [m]
    cd* coherency;           // [n_bins][a][a] or NULL
    double* magnitude;       // [n_bins][a][a] or NULL
    double* multiple;        // [n_bins][a] or NULL
    int32_t* fail;           // [2]: failed problems, (problem, kept signal) cases without a residual
};

__host__ __device__ constexpr size_t pg_lds_bytes(int64_t a, int64_t m) {
    return ((size_t)m * (m + 1) / 2 + (size_t)m * a) * sizeof(cd) + (size_t)(2 * a + m) * sizeof(double) + 16;
}

__global__ __launch_bounds__(PC_THREADS) void partial_given_kernel(PartialGivenArgs g) {
    extern __shared__ __attribute__((aligned(16))) char pc_smem[];
    const int a = g.a, m = g.m, tid = threadIdx.x;
    cd* P = reinterpret_cast<cd*>(pc_smem);
    cd* W = P + m * (m + 1) / 2;
    double* dz = reinterpret_cast<double*>(W + m * a);
    double* da = dz + m;
    double* r = da + a;
    int* bad = reinterpret_cast<int*>(r + a);
    const double qnan = nan("");
    // entry e = tid + 256 s of an [rows][a] array is (k0 + s q + carries, i): no division per entry
    const int q = PC_THREADS / a, rm = PC_THREADS - q * a;
    const int k0 = tid / a, i0 = tid - k0 * a;

    for (int64_t bin = blockIdx.x; bin < g.n_bins; bin += gridDim.x) {
        const ScRec rec = sc_csm_record(g.accum, g.v, 0, bin);
        if (tid == 0) *bad = 0;
        __syncthreads();
        // 1. the diagonal of the given and the kept signals; an index outside the record fails the problem unread
        for (int t = tid; t < m + a; t += PC_THREADS) {
            const int c = t < m ? g.given[t] : g.kept[t - m];
            bool ok = c >= 0 && c < g.n_signals;
            double s = 1.0;
            if (ok) {
                s = sc_csm_entry(rec, g.v, c, c).x;
                ok = s > 0.0 && isfinite(s);
            }
            if (!ok) *bad = 1;
            dz[t] = ok ? s : 1.0;
        }
        __syncthreads();
        if (!*bad) {
            // the Z block and B = S'_ZA, scaled to the unit diagonal
            for (int e = tid; e < m * m; e += PC_THREADS) {
                const int j = e / m, i = e - j * m;
                if (i > j) {
                    const cd s = sc_csm_entry(rec, g.v, g.given[i], g.given[j]);
                    const double w = sqrt(dz[i] * dz[j]);
                    P[pc_row(i) + j] = make_double2(s.x / w, s.y / w);
                } else if (i == j) {
                    P[pc_row(i) + i] = make_double2(1.0, 0.0);
                }
            }
            for (int k = k0, i = i0; k < m;) {
                const cd s = sc_csm_entry(rec, g.v, g.given[k], g.kept[i]);
                const double w = sqrt(dz[k] * da[i]);
                W[k * a + i] = make_double2(s.x / w, s.y / w);
                i += rm; k += q;
                if (i >= a) { i -= a; ++k; }
            }
        }
        __syncthreads();
        // 2. Cholesky S'_ZZ = L L^H
        if (PC_STEPS >= 2 && !*bad) pc_cholesky_packed(P, m, (double)m * 0x1p-52, bad);
        __syncthreads();
        const bool failed = *bad != 0;
        if (!failed && PC_STEPS >= 3) {
            // 3. L W = B.  Iteration k: rows k' > k lose L_k'k W_k with W_k = B_k / L_kk formed on the fly from the unscaled row,
            // and row k - 1 (read by nobody now) is scaled; two entries a thread and step with their loads ahead of the first store
            double rprev = 1.0;
            for (int k = 0; k < m; ++k) {
                const double rk = 1.0 / P[pc_row(k) + k].x;
                if (k > 0)
                    for (int i = tid; i < a; i += PC_THREADS) {
                        const cd v = W[(k - 1) * a + i];
                        W[(k - 1) * a + i] = make_double2(v.x * rprev, v.y * rprev);
                    }
                const cd* wk = W + k * a;
                for (int kk = k + 1 + k0, i = i0; kk < m;) {
                    int kk2 = kk + q, i2 = i + rm;
                    if (i2 >= a) { i2 -= a; ++kk2; }
                    const bool two = kk2 < m;
                    if (!two) { kk2 = kk; i2 = i; }
                    const cd l = P[pc_row(kk) + k], b = wk[i], v = W[kk * a + i];
                    const cd l2 = P[pc_row(kk2) + k], b2 = wk[i2], v2 = W[kk2 * a + i2];
                    const double tx = b.x * rk, ty = b.y * rk, tx2 = b2.x * rk, ty2 = b2.y * rk;
                    W[kk * a + i] = make_double2(v.x - (l.x * tx - l.y * ty), v.y - (l.x * ty + l.y * tx));
                    if (two) W[kk2 * a + i2] = make_double2(v2.x - (l2.x * tx2 - l2.y * ty2), v2.y - (l2.x * ty2 + l2.y * tx2));
                    kk = kk2 + q; i = i2 + rm;
                    if (i >= a) { i -= a; ++kk; }
                    if (!two) break;
                }
                __syncthreads();
                rprev = rk;
            }
            for (int i = tid; i < a; i += PC_THREADS) {
                const cd v = W[(m - 1) * a + i];
                W[(m - 1) * a + i] = make_double2(v.x * rprev, v.y * rprev);
            }
            __syncthreads();
            // 4. r_i = 1 - sum_k |W_ki|^2 and R_i; a kept signal that the given ones explain entirely
            if (PC_STEPS >= 4)
                for (int i = tid; i < a; i += PC_THREADS) {
                    double s = 0.0;
                    int k = 0;
                    for (; k + 3 < m; k += 4) {
                        cd w[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) w[u] = W[(k + u) * a + i];
#pragma unroll
                        for (int u = 0; u < 4; ++u) s += w[u].x * w[u].x + w[u].y * w[u].y;
                    }
                    for (; k < m; ++k) {
                        const cd w = W[k * a + i];
                        s += w.x * w.x + w.y * w.y;
                    }
                    const double ri = 1.0 - s;
                    const bool none = !(ri > (double)(m + 1) * 0x1p-52) || !isfinite(ri);
                    r[i] = none ? qnan : 1.0 / sqrt(ri);           // (the two square roots per kept signal here, not per pair in step 5)
                    da[i] = 1.0 / sqrt(da[i]);
                    if (none) atomicAdd(g.fail + 1, 1);
                    if (g.multiple) g.multiple[bin * a + i] = none ? 1.0 : sqrt(s);
                }
            __syncthreads();
        }
        // 5. outputs (6.: NaN everywhere for a failed problem): tile (ti >= tj) of 8 x 8 pairs per wave and step
        cd* oc = g.coherency ? g.coherency + bin * a * a : nullptr;
        double* om = g.magnitude ? g.magnitude + bin * a * a : nullptr;
        const int wave = tid >> 6, li = (tid >> 3) & 7, lj = tid & 7;
        const int T = (a + 7) >> 3, n_tiles = T * (T + 1) / 2;
        for (int t = wave; t < (PC_STEPS >= 5 ? n_tiles : 0); t += PC_THREADS / 64) {
            int ti, tj;
            pc_unpack(t, ti, tj);
            const int i = 8 * ti + li, j = 8 * tj + lj;
            if (i >= a || j > i) continue;
            double gx = qnan, gy = qnan;
            if (!failed && i != j) {
                const cd s = sc_csm_entry(rec, g.v, g.kept[i], g.kept[j]);
                double sx = 0.0, sy = 0.0;                         // conj(W_ki) W_kj
                int k = 0;
                for (; k + 3 < m; k += 4) {
                    cd p[4], q4[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { p[u] = W[(k + u) * a + i]; q4[u] = W[(k + u) * a + j]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        sx += p[u].x * q4[u].x + p[u].y * q4[u].y;
                        sy += p[u].x * q4[u].y - p[u].y * q4[u].x;
                    }
                }
                for (; k < m; ++k) {
                    const cd p = W[k * a + i], q1 = W[k * a + j];
                    sx += p.x * q1.x + p.y * q1.y;
                    sy += p.x * q1.y - p.y * q1.x;
                }
                const double ws = da[i] * da[j], w = r[i] * r[j];
                gx = (s.x * ws - sx) * w; gy = (s.y * ws - sy) * w;
            }
            if (oc) {
                oc[(int64_t)i * a + j] = make_double2(gx, gy);
                if (i != j) oc[(int64_t)j * a + i] = make_double2(gx, -gy);
            }
            if (om) {
                const double mag = i == j ? qnan : sqrt(gx * gx + gy * gy);
                om[(int64_t)i * a + j] = mag;
                if (i != j) om[(int64_t)j * a + i] = mag;
            }
        }
        if (failed) {
            if (g.multiple)
                for (int i = tid; i < a; i += PC_THREADS) g.multiple[bin * a + i] = qnan;
            if (tid == 0) atomicAdd(g.fail, 1);
        }
        __syncthreads();                                           // (the next problem overwrites everything)
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

extern "C" int sc_partial_given_max_given(void) { return PG_MAX_GIVEN; }
extern "C" int sc_partial_given_max_kept(void) { return PG_MAX_KEPT; }
extern "C" int64_t sc_partial_given_lds_limit(void) { return (int64_t)PG_LDS_LIMIT; }
extern "C" int64_t sc_partial_given_lds_bytes(int64_t n_kept, int64_t n_given) {
    if (n_kept < 1 || n_kept > PG_MAX_KEPT || n_given < 1 || n_given > PG_MAX_GIVEN) return -1;
    return (int64_t)pg_lds_bytes(n_kept, n_given);
}

extern "C" int sc_partial_coherence_given_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                              int64_t n_observations, const int32_t* d_kept, int n_kept, const int32_t* d_given,
                                              int n_given, void* d_coherency, double* d_magnitude, double* d_multiple,
                                              int32_t* d_fail, void* stream) {
    ScTimed timed_("partial_coherence_given", stream);
    SC_REQUIRE(d_accum && d_fail && d_kept && d_given, "NULL argument");
    SC_REQUIRE(d_coherency || d_magnitude || d_multiple, "no output requested");
    PartialGivenArgs g;
    const int rcv = sc_csm_view(planes, n_bins, n_bins, n_signals, n_observations, &g.v);
    if (rcv != SC_OK) return rcv;
    SC_REQUIRE(n_bins >= 1, "empty problem");
    if (n_given < 1 || n_given > PG_MAX_GIVEN || n_kept < 1 || n_kept > PG_MAX_KEPT || (int64_t)n_kept + n_given > n_signals) {
        sc_set_error("invalid argument: partial coherence given a set takes 1 ... %d given and 1 ... %d kept signals out of the "
                     "%lld of the record (got %d given, %d kept)", PG_MAX_GIVEN, PG_MAX_KEPT, (long long)n_signals, n_given, n_kept);
        return SC_EINVAL;
    }
    // every LDS index of the kernel is a function of (a, m) alone, and pg_lds_bytes(a, m) fits here
    const size_t lds = pg_lds_bytes(n_kept, n_given);
    static_assert(pg_lds_bytes(PG_MAX_KEPT, 8) <= PG_LDS_LIMIT && pg_lds_bytes(512, 16) <= PG_LDS_LIMIT &&
                  pg_lds_bytes(1, PG_MAX_GIVEN) <= PG_LDS_LIMIT, "the advertised sizes must fit LDS");
    if (lds > PG_LDS_LIMIT) {
        sc_set_error("invalid argument: %d kept signals given %d need %lld bytes of LDS, beyond the %lld of a compute unit", n_kept,
                     n_given, (long long)lds, (long long)PG_LDS_LIMIT);
        return SC_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    g.accum = sc_rec(d_accum, planes); g.a = n_kept; g.m = n_given; g.n_signals = (int)n_signals; g.n_bins = n_bins;
    g.kept = d_kept; g.given = d_given;
    g.coherency = static_cast<cd*>(d_coherency); g.magnitude = d_magnitude; g.multiple = d_multiple; g.fail = d_fail;
    SC_CHECK_HIP(hipMemsetAsync(d_fail, 0, 8, st));
    if (lds > 64 * 1024)
        SC_CHECK_HIP(hipFuncSetAttribute((const void*)partial_given_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // persistent workgroups: as many a compute unit as their LDS allows (at most 8: 2048 threads)
    int per_cu = (int)(PG_LDS_LIMIT / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int64_t want = (int64_t)256 * per_cu;
    const unsigned blocks = (unsigned)(n_bins < want ? n_bins : want);
    hipLaunchKernelGGL(partial_given_kernel, dim3(blocks), dim3(PC_THREADS), lds, st, g);
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}
