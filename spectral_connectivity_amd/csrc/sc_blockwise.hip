// sc_blockwise.hip -- blockwise spectral Granger prediction (Geweke 1982, multivariate form): how much block b of signals
// predicts block a, frequency by frequency, for pairs of signal blocks.
//
// For a pair (a, b) with n_a + n_b = m signals, ordered a first, then b: S(f) the m x m two-sided spectrum, Psi(f) its Wilson
// factor, Psi0 = Re mean_n Psi(f), Sigma = Psi0 Psi0^T, H = Psi Psi0^-1.  Geweke's measure
//     F_{b -> a}(f) = ln det S_aa(f) - ln det(S_aa(f) - H_ab Sigma~_bb H_ab^H),  Sigma~_bb = Sigma_bb - Sigma_ba Sigma_aa^-1 Sigma_ab
// needs no inverse: with U_b (m x n_b) any orthonormal basis of the null space of the rows Psi0[a, :] (LQ factorisation
// Psi0 = L Q^T: Sigma~_bb = L_bb L_bb^T and Psi0^-1[:, b] L_bb = Q[:, b]; V V^H is invariant under U_b -> U_b O),
//     H_ab Sigma~_bb H_ab^H = V_a V_a^H,   V_a(f) = Psi[a, :](f) U_b,
// and alike F_{a -> b} with V_b = Psi[b, :](f) U_a, U_a orthogonal to the rows Psi0[b, :].  With n_a = n_b = 1 this is the
// pairwise measure.  The device work of a batch of pairs that share m, over G groups (windows x kept axes):
//   bw_gather        the two-sided spectra [pairs G][N][m][m] from the CSM records (or from caller spectra), by index lists
//   sc_mvar_factor_f64 over the pairs G problems, unchanged (sc_mvar.hip)
//   bw_nullspace     Psi0 and R = [U_a | U_b] per problem: Householder QR of Psi0[a, :]^T and Psi0[b, :]^T, the last n_b / n_a
//                    columns of the full Q (per window, not per bin)
//   product          Y = Psi(f) R per (problem, non-negative bin) on the fp64 matrix cores (sc_mvar.hip's launcher):
//                    V_a = Y[a, n_a:], V_b = Y[b, :n_a]
//   bw_epilogue      per (bin, problem, direction): Cholesky log-determinants of S_tt and S_tt - V_t V_t^H (sc_wg_cholesky), F =
//                    their difference
// Non-positive-definite blocks and values <= 0 are NaN (the pairwise measure's convention).
#include <math.h>
#include <vector>
#include "sc_common.h"
#include "sc_workspace.h"

#define BW_LDS_BLOCK 64          // blocks of up to this many signals are factored in LDS by the epilogue, larger ones in place
#define BW_LDS_NULLSPACE 64      // problems of up to this many signals keep Psi0 in LDS in bw_nullspace

struct BwDims {
    int64_t G, N;                // groups, two-sided length
    int C, m;                    // signals of the records / spectra, signals of a problem
    ScCsmView v;                 // the records (d_accum)
};

// S2[q G + g][n][r][c] = S_g(n)[members[q][r]][members[q][c]] for pair q.  From the records or from S [G][N][C][C].
__global__ void __launch_bounds__(256) bw_gather(ScRec accum, const cd* __restrict__ S, BwDims d, const int32_t* __restrict__ members,
                                                 cd* __restrict__ S2) {
    const int m = d.m, E = m * m;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int64_t p = blockIdx.z;
    if (e >= E) return;
    const int64_t g = p % d.G, q = p / d.G;
    const int r = e / m, c = e - r * m;
    const int i = members[q * m + r], j = members[q * m + c];
    for (int64_t n = blockIdx.y; n < d.N; n += gridDim.y) {
        const cd v = S ? S[((g * d.N + n) * d.C + i) * d.C + j] : sc_csm_two_sided(accum, d.v, g, n, i, j);
        S2[(p * d.N + n) * E + e] = v;
    }
}

// Householder QR of the k columns x_c = A[(r0 + c) m + 0 .. m-1] (rows r0 .. r0+k-1 of Psi0, row-major): reflector j,
// H_j = I - beta_j v_j v_j^T, overwrites x_j[j .. m-1] with v_j; beta[r0 + j] = beta_j.
__device__ void bw_householder(double* A, int m, int r0, int k, double* beta, double* red4) {
    const int tid = threadIdx.x;
    for (int j = 0; j < k; ++j) {
        double* x = A + (int64_t)(r0 + j) * m;
        double s = 0.0;
        for (int r = j + tid; r < m; r += 256) s = fma(x[r], x[r], s);
        s = sc_wg_sum(s, red4, tid);
        if (tid == 0) {
            const double x0 = x[j], alpha = -copysign(sqrt(s), x0), v0 = x0 - alpha;
            const double vtv = s - x0 * x0 + v0 * v0;
            beta[r0 + j] = vtv > 0.0 ? 2.0 / vtv : 0.0;
            x[j] = v0;
        }
        __syncthreads();
        const double bj = beta[r0 + j];
        for (int c = j + 1 + tid; c < k; c += 256) {
            double* y = A + (int64_t)(r0 + c) * m;
            double dot = 0.0;
            for (int r = j; r < m; ++r) dot = fma(x[r], y[r], dot);
            dot *= bj;
            for (int r = j; r < m; ++r) y[r] = fma(-dot, x[r], y[r]);
        }
        __syncthreads();
    }
}

// One workgroup per problem p = q G + g (n_a = split[q]):
//   Psi0 = Re mean_n Psi[p][n]  (LDS up to BW_LDS_NULLSPACE signals, beyond the problem's slice of `scratch`)
//   R[p] = [U_a | U_b]: column c < n_a is column n_b + c of the full Q of Psi0[b, :]^T, column c >= n_a column c of that of
//   Psi0[a, :]^T (Q e = H_0 H_1 ... H_{k-1} e), real, written as complex128 m x m row-major.
__global__ void __launch_bounds__(256) bw_nullspace(const cd* __restrict__ Psi, const int32_t* __restrict__ split, int64_t G, int64_t N,
                                                    int m, int in_lds, double* __restrict__ scratch, cd* __restrict__ R) {
    extern __shared__ double bw_psi0[];
    __shared__ double beta[512];
    __shared__ double red4[4];
    const int tid = threadIdx.x, E = m * m;
    const int64_t p = blockIdx.x;
    const int na = split[p / G], nb = m - na;
    double* A = in_lds ? bw_psi0 : scratch + p * E;
    const cd* x = Psi + p * N * E;
    for (int e = tid; e < E; e += 256) {
        double s = 0.0;
        for (int64_t n = 0; n < N; ++n) s += x[n * E + e].x;
        A[e] = s / (double)N;
    }
    __syncthreads();
    bw_householder(A, m, 0, na, beta, red4);
    bw_householder(A, m, na, nb, beta, red4);
    cd* Rp = R + p * E;
    for (int c = tid; c < m; c += 256) {
        const int r0 = c < na ? na : 0, k = c < na ? nb : na, unit = c < na ? nb + c : c;
        for (int r = 0; r < m; ++r) Rp[r * m + c] = make_double2(r == unit ? 1.0 : 0.0, 0.0);
        for (int j = k - 1; j >= 0; --j) {
            const double* v = A + (int64_t)(r0 + j) * m;
            double dot = 0.0;
            for (int r = j; r < m; ++r) dot = fma(v[r], Rp[r * m + c].x, dot);
            dot *= beta[r0 + j];
            for (int r = j; r < m; ++r) Rp[r * m + c].x = fma(-dot, v[r], Rp[r * m + c].x);
        }
    }
}

// ln det of a Hermitian positive-definite matrix from its Cholesky factor: 2 sum ln L[k][k] (workgroup sum)
__device__ double bw_logdet(const cd* L, int ld, int n, double* red4) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += log(L[k * ld + k].x);
    return 2.0 * sc_wg_sum(s, red4, threadIdx.x);
}

// One workgroup per (bin f, problem p = q G + g, direction): target block t (dir 0: a, rows 0 .. n_a-1; dir 1: b), the other o.
//   V = Y[t rows, o columns] (Y = Psi(f) R),  D = S_tt - V V^H
//   out[g][f][t block][o block] = ln det S_tt - ln det D, NaN where a Cholesky pivot is not positive or the value is not positive.
// Blocks of up to lds_max signals are factored in LDS; larger ones in place in S2 (the lower triangle of S_tt; its strict upper
// triangle stays, the diagonal is saved first -- the two directions of a problem touch disjoint diagonal blocks).
__global__ void __launch_bounds__(256) bw_epilogue(cd* __restrict__ S2, const cd* __restrict__ Y, const int32_t* __restrict__ split,
                                                   const int32_t* __restrict__ cell, int64_t G, int64_t N, int64_t F, int m,
                                                   int64_t n_blocks, int lds_max, double* __restrict__ out) {
    extern __shared__ cd bw_block[];
    __shared__ double diag[512];
    __shared__ double red4[4];
    __shared__ int bad;
    const int tid = threadIdx.x, E = m * m;
    const int64_t f = blockIdx.x, p = blockIdx.y, q = p / G, g = p - q * G;
    const int dir = blockIdx.z, na = split[q];
    const int t0 = dir ? na : 0, nt = dir ? m - na : na, o0 = dir ? 0 : na, no = m - nt;
    cd* Sb = S2 + (p * N + f) * E;
    const cd* Yb = Y + (p * F + f) * E;
    const bool lds = nt <= lds_max;
    cd* L = lds ? bw_block : Sb + t0 * m + t0;
    const int ld = lds ? nt : m;
    if (tid == 0) bad = 0;
    for (int i = tid; i < nt; i += 256) diag[i] = Sb[(int64_t)(t0 + i) * (m + 1)].x;
    if (lds)
        for (int e = tid; e < nt * nt; e += 256) {
            const int i = e / nt, j = e - i * nt;
            if (j <= i) L[i * ld + j] = Sb[(t0 + i) * m + t0 + j];
        }
    __syncthreads();
    sc_wg_cholesky(L, ld, nt, &bad);
    const double logdet_s = bw_logdet(L, ld, nt, red4);
    for (int e = tid; e < nt * nt; e += 256) {
        const int i = e / nt, j = e - i * nt;
        if (j > i) continue;
        double re, im;
        if (i == j) { re = diag[i]; im = 0.0; }
        else { const cd s = Sb[(t0 + j) * m + t0 + i]; re = s.x; im = -s.y; }
        const cd* vi = Yb + (t0 + i) * m + o0;
        const cd* vj = Yb + (t0 + j) * m + o0;
        for (int k = 0; k < no; ++k) {                     // - V[i][k] conj(V[j][k])
            const cd a = vi[k], b = vj[k];
            re -= a.x * b.x + a.y * b.y;
            im -= a.y * b.x - a.x * b.y;
        }
        L[i * ld + j] = make_double2(re, im);
    }
    __syncthreads();
    sc_wg_cholesky(L, ld, nt, &bad);
    const double logdet_d = bw_logdet(L, ld, nt, red4);
    if (tid == 0) {
        const int a = cell[2 * q], b = cell[2 * q + 1];
        const int ti = dir ? b : a, si = dir ? a : b;
        const double val = logdet_s - logdet_d;
        out[((g * F + f) * n_blocks + ti) * n_blocks + si] = (!bad && val > 0.0) ? val : nan("");
    }
}

// The workspace of one call with P = n_pairs G problems of m signals (ws_blockwise of sc_workspace.h) on d_work, or counted only
static int bw_layout(void* d_work, int64_t P, int64_t m, int64_t N, WsBlockwise<cd>* k, size_t* need) {
    if (m < 2 || m > sc_mvar_max_signals()) {
        sc_set_error("blockwise Granger: 2 <= signals of a block pair <= %d (got %lld)", sc_mvar_max_signals(), (long long)m);
        return SC_EUNSUPPORTED;
    }
    size_t mvar = 0;
    const int rc = sc_mvar_workspace_bytes(P, m, N, &mvar);
    if (rc != SC_OK) return rc;
    ScCarver w(d_work);
    *k = ws_blockwise<cd>(w, P, m, N, mvar);
    *need = w.used;
    return SC_OK;
}

extern "C" int sc_blockwise_granger_workspace_bytes(int64_t n_groups, int64_t m, int64_t N, int64_t n_pairs, size_t* bytes) {
    SC_REQUIRE(bytes && n_groups >= 1 && n_pairs >= 1 && N >= 2, "bad workspace query");
    WsBlockwise<cd> k;
    return bw_layout(nullptr, n_groups * n_pairs, m, N, &k, bytes);
}

extern "C" int sc_blockwise_granger_f64(const void* d_accum, const void* d_S, int64_t n_groups, int64_t n_freq_accum, int64_t N,
                                        int64_t C, uint32_t planes, int64_t n_obs, const int32_t* d_members, const int32_t* d_split,
                                        const int32_t* d_cell, int64_t n_pairs, int64_t m, int64_t n_blocks, double tol, int max_iter,
                                        void* d_work, size_t work_bytes, int flags, double* d_out, int32_t* d_n_iter,
                                        int32_t* d_status, int32_t* h_summary, void* stream) {
    ScTimed timed_("blockwise_granger", stream);
    SC_REQUIRE((d_accum != nullptr) != (d_S != nullptr), "pass exactly one of d_accum and d_S");
    SC_REQUIRE(d_members && d_split && d_cell && d_work && d_out && d_n_iter && d_status, "NULL argument");
    SC_REQUIRE(n_groups >= 1 && n_pairs >= 1 && n_groups * n_pairs <= 65535 && N >= 2 && N <= 1 << 24 && C >= 1 && n_blocks >= 2,
               "bad problem size");
    WsBlockwise<cd> k;
    size_t need = 0;
    int rc = bw_layout(d_work, n_groups * n_pairs, m, N, &k, &need);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(work_bytes >= need, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    // the index lists address the records and the output: read back and checked before any launch reads them
    std::vector<int32_t> members((size_t)(n_pairs * m)), split((size_t)n_pairs), cell((size_t)(2 * n_pairs));
    SC_CHECK_HIP(hipMemcpyAsync(members.data(), d_members, members.size() * 4, hipMemcpyDeviceToHost, st));
    SC_CHECK_HIP(hipMemcpyAsync(split.data(), d_split, split.size() * 4, hipMemcpyDeviceToHost, st));
    SC_CHECK_HIP(hipMemcpyAsync(cell.data(), d_cell, cell.size() * 4, hipMemcpyDeviceToHost, st));
    SC_CHECK_HIP(hipStreamSynchronize(st));
    int max_block = 0;
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int na = split[q];
        SC_REQUIRE(na >= 1 && na < m, "every pair needs 1 <= n_a < m");
        SC_REQUIRE(cell[2 * q] >= 0 && cell[2 * q] < n_blocks && cell[2 * q + 1] >= 0 && cell[2 * q + 1] < n_blocks &&
                   cell[2 * q] != cell[2 * q + 1], "output block indices outside [0, n_blocks) or equal");
        max_block = na > max_block ? na : max_block;
        max_block = m - na > max_block ? (int)(m - na) : max_block;
    }
    for (int32_t s : members) SC_REQUIRE(s >= 0 && s < C, "member signal outside [0, n_signals)");
    const int64_t G = n_groups, P = G * n_pairs, F = N / 2 + 1, E = m * m;
    cd *S2 = k.S2, *Psi = k.Psi, *R = k.R, *Y = k.Y;
    if (!(flags & SC_BLOCKWISE_KEEP_OUTPUT)) sc_internal_fill_nan(d_out, G * F * n_blocks * n_blocks, st);
    BwDims d = {};
    d.G = G; d.N = N; d.C = (int)C; d.m = (int)m;
    if (d_accum && (rc = sc_csm_view(planes, n_freq_accum, N, C, n_obs, &d.v)) != SC_OK) return rc;
    const dim3 gridG((unsigned)((E + 255) / 256), (unsigned)(N < 1024 ? N : 1024), (unsigned)P);
    hipLaunchKernelGGL(bw_gather, gridG, dim3(256), 0, st, sc_rec(d_accum, planes), (const cd*)d_S, d, d_members, S2);
    SC_CHECK_HIP(hipGetLastError());
    // factors of the pair spectra: the full factorisation's own path over the P problems
    if ((rc = sc_mvar_factor_f64(nullptr, S2, P, 0, N, m, 0, 1, tol, max_iter, k.mvar, k.mvar_bytes, Psi, d_n_iter, d_status, h_summary,
                                 stream)) != SC_OK)
        return rc;
    // (the factorisation has synchronised the stream: its workspace is free again and holds R, Y and psi0 from here on)
    const int ns_lds = m <= BW_LDS_NULLSPACE;
    hipLaunchKernelGGL(bw_nullspace, dim3((unsigned)P), dim3(256), ns_lds ? (size_t)E * sizeof(double) : 0, st, (const cd*)Psi, d_split,
                       G, N, (int)m, ns_lds, k.psi0, R);
    SC_CHECK_HIP(hipGetLastError());
    // Y = Psi(f) R on the non-negative bins
    if ((rc = sc_internal_mvar_gemm(m, P, F, Psi, N * E, E, R, E, 0, Y, F * E, E, st)) != SC_OK) return rc;
    const int lds_max = max_block < BW_LDS_BLOCK ? max_block : BW_LDS_BLOCK;
    const size_t lds = (size_t)lds_max * lds_max * sizeof(cd);
    SC_CHECK_HIP(hipFuncSetAttribute((const void*)bw_epilogue, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bw_epilogue, dim3((unsigned)F, (unsigned)P, 2), dim3(256), lds, st, S2, (const cd*)Y, d_split, d_cell, G, N, F,
                       (int)m, n_blocks, lds_max, d_out);
    return sc_sync_or_report(st, "blockwise Granger epilogue");
}
