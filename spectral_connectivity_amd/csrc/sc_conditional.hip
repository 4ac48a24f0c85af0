// sc_conditional.hip -- conditional spectral Granger prediction (Geweke 1984; Ding, Chen & Bressler 2006, section 3.3):
// j -> i given every other signal, for all ordered pairs, from the full minimum-phase factor and one reduced factorisation
// per dropped signal.
//
// For target i, source j and the conditioning set z = the rest, with Psi(f) the full factor (two-sided, N bins), Psi0 =
// Re mean_n Psi(f), Sigma = Psi0 Psi0^T, and Phi(f) the factor of the spectrum with row and column j removed (Phi0, Sigma^r
// alike), the normalisations of Ding et al. (P1 / P2 of the full model, the rotation of the reduced one, Q = G~ext^-1 H~)
// collapse to
//     M(f) = Psi(f) Psi0^T                      (= H(f) Sigma: the first column of P^-1 is Sigma[:, i] / Sigma[i, i])
//     v_i(f) = [Phi0 Phi(f)^-1 M(f)[rows != j, col i]]  at the row of i in the reduced system
//     F_{j -> i | rest}(f) = ln(Sigma^r[i, i] Sigma[i, i] / |v_i(f)|^2)
// (no inverse of Psi0, no Tikhonov term).  The device work of a chunk of D dropped signals and G groups:
//   cg_gather       the reduced two-sided spectra [D G][N][C-1][C-1] from the CSM records (or from caller spectra)
//   sc_mvar_factor_f64 over the D G reduced problems, unchanged (sc_mvar.hip)
//   cg_lag0         Psi0^T per group and Phi0 per reduced problem (complex, zero imaginary part: operands of the products)
//   products        M = Psi(f) Psi0^T per (group, bin); Phi(f)^-1 (register-resident Gauss-Jordan up to 64 signals, matrix-core /
//                   blocked inverses beyond); K = Phi0 Phi(f)^-1 on the fp64 matrix cores (sc_mvar.hip's launchers)
//   cg_epilogue     v_i = sum_k K[r(i), k] M[k^, i] (k^: the full index of reduced index k), one wave per i, and F
// The reduced problems of a chunk share one workspace; the host walks long lists of dropped signals in chunks
// (SC_CONDITIONAL_KEEP_OUTPUT), like the pair lists of sc_granger_pairwise_f64.
#include <math.h>
#include "sc_common.h"
#include "sc_workspace.h"

struct CgDims {
    int64_t G, N;        // groups, two-sided length
    int C;
    ScCsmView v;         // the records (d_accum)
};

__device__ __forceinline__ int cg_full(int k, int j) { return k < j ? k : k + 1; }     // reduced index -> full index

// S_red[d G + g][n][a][b] = S_g(n)[a^][b^] with a^, b^ skipping the dropped signal dropped[d].  From the records (upper-triangular
// 16 x 16 tiles of un-normalised sums; real input: S(-f) = conj S(f) completes the bins past N/2) or from S [G][N][C][C].
__global__ void __launch_bounds__(256) cg_gather(ScRec accum, const cd* __restrict__ S, CgDims d, const int32_t* __restrict__ dropped,
                                                 cd* __restrict__ Sred) {
    const int Cr = d.C - 1, Er = Cr * Cr;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int64_t pr = blockIdx.z;                   // reduced problem d G + g
    if (e >= Er) return;
    const int64_t g = pr % d.G;
    const int jd = dropped[pr / d.G];
    if (jd < 0 || jd >= d.C) return;                 // (an index outside the signals drops nothing)
    const int a = e / Cr, b = e - a * Cr;
    const int i = cg_full(a, jd), j = cg_full(b, jd);
    for (int64_t n = blockIdx.y; n < d.N; n += gridDim.y) {
        cd v;
        if (S) {
            v = S[((g * d.N + n) * d.C + i) * d.C + j];
        } else {
            v = sc_csm_two_sided(accum, d.v, g, n, i, j);
        }
        Sred[(pr * d.N + n) * Er + e] = v;
    }
}

// out[p][e] = Re mean_n X[p][n][e] as a complex number with zero imaginary part (transpose: out[p][b C + a] of element a C + b)
__global__ void __launch_bounds__(256) cg_lag0(const cd* __restrict__ X, cd* __restrict__ out, int64_t N, int C, int transpose) {
    const int E = C * C;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (e >= E) return;
    const cd* x = X + p * N * E + e;
    double s = 0.0;
    for (int64_t n = 0; n < N; ++n) s += x[n * E].x;
    const int a = e / C, b = e - a * C;
    out[p * E + (transpose ? b * C + a : e)] = make_double2(s / (double)N, 0.0);
}

// One workgroup per (bin f, group g, dropped signal d), one wave per target i != j (reduced row r):
//   v = sum_k K[r][k] M[k^][i]     Sigma^r[r][r] = sum_k Phi0[r][k]^2     Sigma[i][i] = sum_l Psi0[i][l]^2 (= Psi0^T[l][i]^2)
//   out[g][f][i][j] = ln(Sigma^r Sigma / |v|^2), NaN where that is not positive (the pairwise measure's convention)
__global__ void __launch_bounds__(256) cg_epilogue(const cd* __restrict__ K, const cd* __restrict__ M, const cd* __restrict__ Phi0,
                                                   const cd* __restrict__ Psi0T, const int32_t* __restrict__ dropped, int64_t G,
                                                   int64_t F, int64_t N, int C, double* __restrict__ out) {
    const int Cr = C - 1, Er = Cr * Cr, E = C * C;
    const int64_t f = blockIdx.x, g = blockIdx.y, d = blockIdx.z;
    const int64_t pr = d * G + g;
    const int jd = dropped[d];
    if (jd < 0 || jd >= C) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const cd* Kb = K + (pr * N + f) * Er;            // K lives at the bin slots of the factor's layout (bin stride Er, problem N Er)
    const cd* Mb = M + (g * F + f) * E;
    const cd* P0 = Phi0 + pr * Er;
    const cd* Q0 = Psi0T + g * E;
    for (int r = wave; r < Cr; r += 4) {
        const int i = cg_full(r, jd);
        double vr = 0.0, vi = 0.0, sr = 0.0, sf = 0.0;
        for (int k = lane; k < Cr; k += 64) {
            const cd kv = Kb[r * Cr + k], mv = Mb[cg_full(k, jd) * C + i];
            vr = fma(kv.x, mv.x, fma(-kv.y, mv.y, vr));
            vi = fma(kv.x, mv.y, fma(kv.y, mv.x, vi));
            const double p0 = P0[r * Cr + k].x;
            sr = fma(p0, p0, sr);
        }
        for (int l = lane; l < C; l += 64) {
            const double q0 = Q0[l * C + i].x;
            sf = fma(q0, q0, sf);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            vr += __shfl_xor(vr, off);
            vi += __shfl_xor(vi, off);
            sr += __shfl_xor(sr, off);
            sf += __shfl_xor(sf, off);
        }
        if (lane == 0) {
            const double val = log(sr * sf / (vr * vr + vi * vi));
            out[((g * F + f) * C + i) * C + jd] = val > 0.0 ? val : nan("");
        }
    }
}

// The workspace of one call with D dropped signals (ws_conditional of sc_workspace.h) on d_work, or counted only (d_work NULL)
static int cg_layout(void* d_work, int64_t G, int64_t C, int64_t N, int64_t D, WsConditional<cd>* k, size_t* need) {
    if (C < 2 || C > sc_mvar_max_signals()) {
        sc_set_error("conditional Granger: 2 <= n_signals <= %d (got %lld)", sc_mvar_max_signals(), (long long)C);
        return SC_EUNSUPPORTED;
    }
    size_t mvar = 0;
    const int rc = sc_mvar_workspace_bytes(G * D, C - 1, N, &mvar);
    if (rc != SC_OK) return rc;
    ScCarver w(d_work);
    *k = ws_conditional<cd>(w, G, C, N, D, mvar);
    *need = w.used;
    return SC_OK;
}

extern "C" int sc_conditional_granger_workspace_bytes(int64_t n_groups, int64_t C, int64_t N, int64_t n_dropped, size_t* bytes) {
    SC_REQUIRE(bytes && n_groups >= 1 && n_dropped >= 1 && N >= 2, "bad workspace query");
    WsConditional<cd> k;
    return cg_layout(nullptr, n_groups, C, N, n_dropped, &k, bytes);
}

extern "C" int sc_conditional_granger_f64(const void* d_accum, const void* d_S, int64_t n_groups, int64_t n_freq_accum, int64_t N,
                                          int64_t C, uint32_t planes, int64_t n_obs, const void* d_G, const int32_t* d_dropped,
                                          int64_t n_dropped, double tol, int max_iter, void* d_work, size_t work_bytes, int flags,
                                          double* d_out, int32_t* d_n_iter, int32_t* d_status, int32_t* h_summary, void* stream) {
    ScTimed timed_("conditional_granger", stream);
    SC_REQUIRE((d_accum != nullptr) != (d_S != nullptr), "pass exactly one of d_accum and d_S");
    SC_REQUIRE(d_G && d_dropped && d_work && d_out && d_n_iter && d_status, "NULL argument");
    SC_REQUIRE(n_groups >= 1 && n_dropped >= 1 && n_groups * n_dropped <= 65535 && N >= 2 && N <= 1 << 24, "bad problem size");
    WsConditional<cd> k;
    size_t need = 0;
    int rc = cg_layout(d_work, n_groups, C, N, n_dropped, &k, &need);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(work_bytes >= need, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t G = n_groups, P = G * n_dropped, F = N / 2 + 1, Cr = C - 1;
    const int64_t E = C * C, Er = Cr * Cr;
    cd *Psi0T = k.Psi0T, *M = k.M, *Sred = k.Sred, *Phi = k.Phi, *Phi0 = k.Phi0, *K = k.K;
    if (!(flags & SC_CONDITIONAL_KEEP_OUTPUT)) sc_internal_fill_nan(d_out, G * F * E, st);
    SC_CHECK_HIP(hipMemsetAsync(k.zero, 0, 256, st));
    // reduced spectra
    CgDims d = {};
    d.G = G; d.N = N; d.C = (int)C;
    if (d_accum && (rc = sc_csm_view(planes, n_freq_accum, N, C, n_obs, &d.v)) != SC_OK) return rc;
    const dim3 gridG((unsigned)((Er + 255) / 256), (unsigned)(N < 1024 ? N : 1024), (unsigned)P);
    hipLaunchKernelGGL(cg_gather, gridG, dim3(256), 0, st, sc_rec(d_accum, planes), (const cd*)d_S, d, d_dropped, Sred);
    SC_CHECK_HIP(hipGetLastError());
    // reduced factors: the full factorisation's own path over the D G problems
    if ((rc = sc_mvar_factor_f64(nullptr, Sred, P, 0, N, Cr, 0, 1, tol, max_iter, k.mvar, k.mvar_bytes, Phi, d_n_iter, d_status, h_summary,
                                 stream)) != SC_OK)
        return rc;
    // (the factorisation has synchronised the stream: its workspace is free again and holds Phi0, K and the scratch from here on)
    cd* Phinv = Sred;
    hipLaunchKernelGGL(cg_lag0, dim3((unsigned)((E + 255) / 256), (unsigned)G), dim3(256), 0, st, (const cd*)d_G, Psi0T, N, (int)C, 1);
    hipLaunchKernelGGL(cg_lag0, dim3((unsigned)((Er + 255) / 256), (unsigned)P), dim3(256), 0, st, (const cd*)Phi, Phi0, N, (int)Cr, 0);
    SC_CHECK_HIP(hipGetLastError());
    // M = Psi(f) Psi0^T on the non-negative bins
    if ((rc = sc_internal_mvar_gemm(C, G, F, d_G, N * E, E, Psi0T, E, 0, M, F * E, E, st)) != SC_OK) return rc;
    // Phi(f)^-1, then K = Phi0 Phi(f)^-1 (both at the bin slots of the factor's layout)
    if ((rc = sc_internal_mvar_inverse(Cr, P, N, F, Phi, Phinv, k.scratch, k.zero, st)) != SC_OK) return rc;
    if ((rc = sc_internal_mvar_gemm(Cr, P, F, Phi0, Er, 0, Phinv, N * Er, Er, K, N * Er, Er, st)) != SC_OK) return rc;
    hipLaunchKernelGGL(cg_epilogue, dim3((unsigned)F, (unsigned)G, (unsigned)n_dropped), dim3(256), 0, st, (const cd*)K, (const cd*)M,
                       (const cd*)Phi0, (const cd*)Psi0T, d_dropped, G, F, N, (int)C, d_out);
    return sc_sync_or_report(st, "conditional Granger epilogue");
}
