// sc_canonical.hip -- canonical coherence between groups of channels from the accumulated
// cross-spectral matrix.
//
// Reference (connectivity.py:745-820, :1953-2032): per group g, whiten the (c_g x n_obs)
// coefficient matrix by its thin SVD (A -> U V^H) and take, per group pair, the squared
// largest singular value of (U V^H)_g (U V^H)_h^H -- n_obs-long SVDs per (window, frequency).
// With S = A A^H / n_obs already accumulated by the MFMA kernel the same quantity is
//     sigma_max( L_g^-1 S_gh L_h^-H )^2,     S_gg = L_g L_g^H (Cholesky),
// (identical when every group has full row rank, n_obs >= c_g), i.e.
// per (bin, group pair) two small Cholesky factorisations, two triangular solves and the top
// eigenvalue of a c_g x c_g Hermitian matrix, all fp64.  Three tiers by the largest group of a launch
// (canonical_launch): up to 16 channels a wave per (bin, pair) on factors computed once per bin
// (canonical_factor_kernel + canonical_pair_hh_kernel), up to 64 a persistent workgroup per item with the
// whole problem in LDS, up to 128 the same with the blocks in a global scratch (canonical_big_hh_kernel);
// lambda_max by Householder tridiagonalisation and multisection on the Sturm sequence.  The Jacobi
// kernels of the first rounds (canonical_kernel: one THREAD per item, matrices in per-lane scratch;
// canonical_pair_kernel; canonical_big_kernel) remain behind SC_CANON_EIG=jacobi for cross-checks.
//
// The same kernels give the multivariate imaginary coherence of Ewald, Marzetti, Zappasodi, Meinecke & Nolte 2012
// (NeuroImage 62:1964-1971) through a second READ VIEW of the records (template parameter IM): group blocks Re S_gg, cross
// blocks i Im S_gh.  M = L_a^-1 (i Im S_ab) L_b^-H with L_g L_g^T = Re S_gg has the singular values of
// D = (Re S_aa)^-1/2 Im S_ab (Re S_bb)^-1/2, so lambda_max(M M^H) = MIC^2 and trace(M M^H) = MIM = tr((Re S_aa)^-1 Im S_ab
// (Re S_bb)^-1 Im S_ab^T) -- no other eigen-solver.
#include <math.h>
#include <stdlib.h>
#include "sc_common.h"
#include "sc_jacobi.h"

struct CanonArgs {
    ScRec accum;
    const int32_t* members;   // [G][CMAX] channel indices, -1 padded
    const int32_t* sizes;     // [G]
    double* out;              // [n_bins][G][G]
    int32_t* fail;            // [1] count of (bin, pair) items with a group block that is not positive definite
    ScCsmView v;              // the records (single bins: N = F = n_bins)
    int64_t n_bins;
    int G, n_gpairs;
    int mstride;              // row length of `members` for the workgroup-per-problem kernels (32 or CBIG_C)
    double jtol;
    double* out_mim;          // interaction view: [n_bins][G][G] MIM (`out` then holds MIC)
};

__device__ inline cd csm_read(ScRec rec, const CanonArgs& a, int i, int j) { return sc_csm_entry(rec, a.v, i, j); }

// the records as the kernels read them: S (IM = false: canonical coherence) or the interaction view (IM = true) -- a group
// block entry as (Re S_ij, 0), a cross block entry as (0, Im S_ij)
template <bool IM>
__device__ inline cd csm_group(ScRec rec, const CanonArgs& a, int i, int j) {
    const cd s = csm_read(rec, a, i, j);
    return IM ? make_double2(s.x, 0.0) : s;
}
template <bool IM>
__device__ inline cd csm_cross(ScRec rec, const CanonArgs& a, int i, int j) {
    const cd s = csm_read(rec, a, i, j);
    return IM ? make_double2(0.0, s.y) : s;
}

// interaction view: MIC = sqrt(lambda_max) and MIM = trace(B) of a pair; B is positive semi-definite, so lambda_max <= trace(B)
// (the clamp and the step below keep the rounded MIC x MIC <= MIM to the last bit and make MIC exactly 0 where B is 0).  NaN for
// both when a block failed.
__device__ inline void canon_store_interaction(const CanonArgs& a, int64_t bin, int ga, int gb, double lmax, double tr, bool ok) {
    double mic = ok ? sqrt(fmin(fmax(lmax, 0.0), tr)) : nan("");
    const double mim = ok ? tr : nan("");
    // (the rounded square of a rounded root can lie one unit above its argument: with lambda_max = trace(B), a group of one
    //  channel, MIC x MIC came out above MIM in the last bit; one step down is enough with a correctly rounded root, the
    //  square moves by two units of the root's)
    for (int k = 0; k < 2 && ok && __dmul_rn(mic, mic) > tr; ++k) mic = nextafter(mic, 0.0);
    double* o = a.out + bin * a.G * a.G;
    double* p = a.out_mim + bin * a.G * a.G;
    o[ga * a.G + gb] = mic;
    o[gb * a.G + ga] = mic;
    p[ga * a.G + gb] = mim;
    p[gb * a.G + ga] = mim;
}

// in-place lower Cholesky of Hermitian positive-definite n x n (row-major, stride CMAX)
template <int CMAX>
__device__ inline bool cholesky(cd (*L)[CMAX], int n) {
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        double d = L[j][j].x;
        for (int k = 0; k < j; ++k) d -= L[j][k].x * L[j][k].x + L[j][k].y * L[j][k].y;
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        const double ljj = sqrt(d);
        L[j][j] = make_double2(ljj, 0.0);
        for (int i = j + 1; i < n; ++i) {
            cd s = L[i][j];
            for (int k = 0; k < j; ++k) { const cd t = zmul_conj(L[i][k], L[j][k]); s.x -= t.x; s.y -= t.y; }
            L[i][j] = make_double2(s.x / ljj, s.y / ljj);
        }
    }
    return ok;
}

template <int CMAX>
__global__ void __launch_bounds__(64) canonical_kernel(CanonArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= a.n_bins * a.n_gpairs) return;
    const int64_t bin = idx / a.n_gpairs;
    int gp = (int)(idx - bin * a.n_gpairs);
    int ga = 0, len = a.G - 1;
    while (gp >= len) { gp -= len; ++ga; --len; }
    const int gb = ga + 1 + gp;
    const int na = a.sizes[ga], nb = a.sizes[gb];
    const int32_t* ma = a.members + ga * CMAX;
    const int32_t* mb = a.members + gb * CMAX;
    const ScRec rec = a.accum + bin * a.v.floats_per_bin;

    cd La[CMAX][CMAX], Lb[CMAX][CMAX], M[CMAX][CMAX];
    for (int i = 0; i < na; ++i)
        for (int j = 0; j <= i; ++j) La[i][j] = csm_read(rec, a, ma[i], ma[j]);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j <= i; ++j) Lb[i][j] = csm_read(rec, a, mb[i], mb[j]);
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) M[i][j] = csm_read(rec, a, ma[i], mb[j]);
    const bool ok = cholesky<CMAX>(La, na) & cholesky<CMAX>(Lb, nb);
    if (!ok) atomicAdd(a.fail, 1);
    // M <- La^-1 M  (forward substitution down the rows)
    for (int j = 0; j < nb; ++j)
        for (int i = 0; i < na; ++i) {
            cd s = M[i][j];
            for (int k = 0; k < i; ++k) { const cd t = zmul(La[i][k], M[k][j]); s.x -= t.x; s.y -= t.y; }
            const double d = La[i][i].x;
            M[i][j] = make_double2(s.x / d, s.y / d);
        }
    // M <- M Lb^-H : row vector y = m Lb^-H  <=>  y conj(Lb)^T = m  (forward substitution along columns)
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) {
            cd s = M[i][j];
            for (int k = 0; k < j; ++k) { const cd t = zmul_conj(M[i][k], Lb[j][k]); s.x -= t.x; s.y -= t.y; }
            const double d = Lb[j][j].x;
            M[i][j] = make_double2(s.x / d, s.y / d);
        }
    // B = M M^H (na x na Hermitian), stored in La
    for (int i = 0; i < na; ++i)
        for (int j = 0; j <= i; ++j) {
            cd s = make_double2(0.0, 0.0);
            for (int k = 0; k < nb; ++k) { const cd t = zmul_conj(M[i][k], M[j][k]); s.x += t.x; s.y += t.y; }
            La[i][j] = s;
            La[j][i] = make_double2(s.x, -s.y);
        }
    // cyclic complex Jacobi, eigenvalues only
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int p = 0; p < na; ++p) {
            dia += La[p][p].x * La[p][p].x;
            for (int q = p + 1; q < na; ++q) off += La[p][q].x * La[p][q].x + La[p][q].y * La[p][q].y;
        }
        if (off <= 1e-30 * dia || off == 0.0) break;
        for (int p = 0; p < na - 1; ++p)
            for (int q = p + 1; q < na; ++q) {
                const cd bpq = La[p][q];
                const double ab = hypot(bpq.x, bpq.y);
                if (ab < 1e-300) continue;
                const cd e = make_double2(bpq.x / ab, bpq.y / ab);       // e^{i phi}
                const double tau = (La[q][q].x - La[p][p].x) / (2.0 * ab);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
                const double c = 1.0 / hypot(1.0, t), s = t * c;
                const cd se = make_double2(s * e.x, s * e.y), sec = make_double2(s * e.x, -s * e.y);
                for (int k = 0; k < na; ++k) {           // columns p, q
                    const cd cp = La[k][p], cq = La[k][q];
                    const cd t1 = zmul(sec, cq), t2 = zmul(se, cp);
                    La[k][p] = make_double2(c * cp.x - t1.x, c * cp.y - t1.y);
                    La[k][q] = make_double2(t2.x + c * cq.x, t2.y + c * cq.y);
                }
                for (int k = 0; k < na; ++k) {           // rows p, q
                    const cd rp = La[p][k], rq = La[q][k];
                    const cd t1 = zmul(se, rq), t2 = zmul(sec, rp);
                    La[p][k] = make_double2(c * rp.x - t1.x, c * rp.y - t1.y);
                    La[q][k] = make_double2(t2.x + c * rq.x, t2.y + c * rq.y);
                }
            }
    }
    double lmax = La[0][0].x;
    for (int p = 1; p < na; ++p) lmax = fmax(lmax, La[p][p].x);
    if (!ok) lmax = nan("");
    double* o = a.out + bin * a.G * a.G;
    o[ga * a.G + gb] = lmax;
    o[gb * a.G + ga] = lmax;
}

// ---- groups of at most 16 channels: factor kernel + pair kernel ------------------------------------
// The thread-per-problem kernel above keeps three 16x16 complex matrices per lane in scratch memory and
// factors every group's block once per PAIR.  Here
//   canonical_factor_kernel  one workgroup per bin, a wave per group: Cholesky factor, inverted in place
//                            (so whitening a pair is two dense 16x16 products with no dependent chains),
//                            written to a [bin][group][16][16] workspace (L2-resident: 4 KB per group);
//   canonical_pair_kernel    a WAVE per (bin, group pair), eight to a workgroup: whitening, B = M M^H
//                            (a lane per entry) and a parallel cyclic Jacobi on B (a lane per 2x2 block of
//                            the round's pairing) in the wave's own 8 KB of LDS, ordered by the wave's
//                            in-order LDS pipe -- no workgroup barrier at all.
// Pair-granular workgroups (7695 at cfg5) fill the 256 CUs evenly and two fit a CU; one workgroup per bin
// with the factors kept in LDS (the first version of this path) left a 513-bin problem waiting for a third
// generation of a single workgroup.
#define CB_C 16
#define CB_WSYNC()                                                  \
    do {                                                            \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      \
        __builtin_amdgcn_wave_barrier();                            \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      \
    } while (0)

__device__ inline cd cb_get(const cd* B, int i, int j) {           // Hermitian, upper triangle stored
    if (i <= j) return B[i * CB_C + j];
    const cd v = B[j * CB_C + i];
    return make_double2(v.x, -v.y);
}
__device__ inline void cb_set(cd* B, int i, int j, cd v) {
    if (i <= j) B[i * CB_C + j] = v;
    else B[j * CB_C + i] = make_double2(v.x, -v.y);
}
__device__ inline double cb_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

#define CB_WAVES 8
#ifndef CB_SWEEPS
#define CB_SWEEPS 12
#endif
template <bool IM>
__global__ void __launch_bounds__(64 * CB_WAVES) canonical_factor_kernel(CanonArgs a, cd* Lg, int* okb) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int G = a.G;
    cd* Ls = reinterpret_cast<cd*>(cb_smem);                                   // [wave][16][16]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t bin = blockIdx.x;
    const ScRec rec = a.accum + bin * a.v.floats_per_bin;

    // phase 1: L_g for every group (a wave per group, left-looking Cholesky, a lane per row)
    for (int g = wave; g < G; g += CB_WAVES) {
        const int n = a.sizes[g];
        const int32_t* mg = a.members + g * CB_C;
        cd* L = Ls + (size_t)wave * CB_C * CB_C;
        for (int e = lane; e < CB_C * CB_C; e += 64) {
            const int i = e / CB_C, j = e % CB_C;
            L[e] = (i < n && j < n) ? csm_group<IM>(rec, a, mg[i], mg[j]) : make_double2(0.0, 0.0);
        }
        CB_WSYNC();
        int ok = 1;
        for (int j = 0; j < n; ++j) {
            double d = L[j * CB_C + j].x;                                   // every lane: the pivot of column j
            for (int k = 0; k < j; ++k) { const cd v = L[j * CB_C + k]; d -= v.x * v.x + v.y * v.y; }
            if (!(d > 0.0)) { ok = 0; d = 1.0; }
            const double ljj = sqrt(d);
            const int i = j + 1 + lane;
            cd s = make_double2(0.0, 0.0);
            if (i < n) {
                s = L[i * CB_C + j];
                for (int k = 0; k < j; ++k) { const cd t = zmul_conj(L[i * CB_C + k], L[j * CB_C + k]); s.x -= t.x; s.y -= t.y; }
            }
            CB_WSYNC();
            if (lane == 0) L[j * CB_C + j] = make_double2(ljj, 0.0);
            if (i < n) L[i * CB_C + j] = make_double2(s.x / ljj, s.y / ljj);
            CB_WSYNC();
        }
        // L <- L^-1 (lower triangular): the whitening of a pair is then two dense 16x16 products with no dependent
        // chains instead of two triangular solves per pair.  Column `lane` of the inverse, top to bottom, kept in
        // registers until every lane is done with L.
        cd inv[CB_C];
#pragma unroll
        for (int i = 0; i < CB_C; ++i) inv[i] = make_double2(0.0, 0.0);
        if (lane < n) {
#pragma unroll
            for (int i = 0; i < CB_C; ++i) {
                if (i >= lane && i < n) {
                    cd sv = make_double2(i == lane ? 1.0 : 0.0, 0.0);
#pragma unroll
                    for (int k = 0; k < CB_C; ++k)
                        if (k >= lane && k < i) { const cd t = zmul(L[i * CB_C + k], inv[k]); sv.x -= t.x; sv.y -= t.y; }
                    const double d = L[i * CB_C + i].x;
                    inv[i] = make_double2(sv.x / d, sv.y / d);
                }
            }
        }
        CB_WSYNC();
        if (lane < CB_C) {
#pragma unroll
            for (int i = 0; i < CB_C; ++i) L[i * CB_C + lane] = (lane < n && i < n) ? inv[i] : make_double2(0.0, 0.0);
        }
        CB_WSYNC();
        cd* out = Lg + ((size_t)bin * G + g) * CB_C * CB_C;
        for (int e = lane; e < CB_C * CB_C; e += 64) out[e] = L[e];
        if (lane == 0) okb[bin * G + g] = ok;
        CB_WSYNC();                                                // L is reused for this wave's next group
    }
}

__global__ void __launch_bounds__(64 * CB_WAVES) canonical_pair_kernel(CanonArgs a, const cd* Lg, const int* okb) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int G = a.G;
    cd* scratch = reinterpret_cast<cd*>(cb_smem);                              // per wave: M, B [16][16]
    double* rot = reinterpret_cast<double*>(scratch + CB_WAVES * 2 * CB_C * CB_C);   // per wave: [8] cos, [8][2] sin
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n_chunks = (a.n_gpairs + CB_WAVES - 1) / CB_WAVES;
    const int64_t bin = blockIdx.x / n_chunks;
    const int chunk = blockIdx.x % n_chunks;
    const ScRec rec = a.accum + bin * a.v.floats_per_bin;
    const cd* Ls = Lg + (size_t)bin * G * CB_C * CB_C;
    const int* okg = okb + bin * G;
    cd* M = scratch + (size_t)wave * 2 * CB_C * CB_C;
    cd* B = M + CB_C * CB_C;
    double* rc = rot + wave * 24;
    cd* rs = reinterpret_cast<cd*>(rc + 8);
    {
        const int pr = chunk * CB_WAVES + wave;
        if (pr >= a.n_gpairs) return;                              // no workgroup barriers below
        int gp = pr, ga = 0, len = G - 1;
        while (gp >= len) { gp -= len; ++ga; --len; }
        const int gb = ga + 1 + gp;
        const int na = a.sizes[ga], nb = a.sizes[gb];
        const int32_t* ma = a.members + ga * CB_C;
        const int32_t* mb = a.members + gb * CB_C;
        const cd* La = Ls + (size_t)ga * CB_C * CB_C;
        const cd* Lb = Ls + (size_t)gb * CB_C * CB_C;
        const bool ok = okg[ga] && okg[gb];
        for (int e = lane; e < CB_C * CB_C; e += 64) {
            const int i = e / CB_C, j = e % CB_C;
            M[e] = (i < na && j < nb) ? csm_read(rec, a, ma[i], mb[j]) : make_double2(0.0, 0.0);
        }
        CB_WSYNC();
        // M <- Linv_a M Linv_b^H as two dense products through B.  The inverse factors come from the workspace (L2):
        // a row of sixteen independent loads per output element, issued together (their upper triangles are zero).
        for (int e = lane; e < CB_C * CB_C; e += 64) {
            const int i = e / CB_C, j = e % CB_C;
            cd la[CB_C];
#pragma unroll
            for (int k = 0; k < CB_C; ++k) la[k] = La[i * CB_C + k];
            cd sv = make_double2(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < CB_C; ++k) { const cd t = zmul(la[k], M[k * CB_C + j]); sv.x += t.x; sv.y += t.y; }
            B[e] = sv;
        }
        CB_WSYNC();
        for (int e = lane; e < CB_C * CB_C; e += 64) {
            const int i = e / CB_C, j = e % CB_C;
            cd lb[CB_C];
#pragma unroll
            for (int k = 0; k < CB_C; ++k) lb[k] = Lb[j * CB_C + k];
            cd sv = make_double2(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < CB_C; ++k) { const cd t = zmul_conj(B[i * CB_C + k], lb[k]); sv.x += t.x; sv.y += t.y; }
            M[e] = sv;
        }
        CB_WSYNC();
        for (int e = lane; e < CB_C * CB_C; e += 64) {      // B = M M^H, both triangles, zero outside na x na
            const int i = e / CB_C, j = e % CB_C;
            cd sv = make_double2(0.0, 0.0);
            if (i < na && j < na) {
#pragma unroll
                for (int k = 0; k < CB_C; ++k) { const cd t = zmul_conj(M[i * CB_C + k], M[j * CB_C + k]); sv.x += t.x; sv.y += t.y; }
                if (i == j) sv.y = 0.0;
            }
            B[e] = sv;
        }
        CB_WSYNC();
        // Parallel cyclic Jacobi, eigenvalues only.  Round r of a sweep pairs the Mp indices by the circle method
        // (index Mp-1 fixed, the others rotating); pair k of the round is rotated by lane k, and lane (u, v) applies
        // B' = J_u^H B J_v to the 2x2 block (pair u) x (pair v).  An odd na pairs one
        // index with the zero row na: zero pivot, identity rotation, no special case.
        const int Mp = na + (na & 1), H = Mp / 2, Q = Mp - 1;
        const bool has_block = lane < H * H;               // every block of the H x H grid has a lane: no mirror writes
        const int bu = has_block ? lane / H : 0, bv = has_block ? lane % H : 0;
        // circle method, kept incrementally: pair k of round r is (r + k, r - k) mod Q, pair 0 is (Q, r); the
        // positions advance by one per round and return to the start after the Q rounds of a sweep
        auto start_x = [Q](int k) { return k == 0 ? Q : k; };
        auto start_y = [Q](int k) { return k == 0 ? 0 : Q - k; };
        auto advance = [Q](int k, int& x, int& y) {
            const int x1 = x + 1, y1 = y + 1;
            if (k != 0) x = x1 == Q ? 0 : x1;
            y = y1 == Q ? 0 : y1;
        };
        int xa = start_x(lane < H ? lane : 0), ya = start_y(lane < H ? lane : 0);
        int xu = start_x(bu), yu = start_y(bu), xv = start_x(bv), yv = start_y(bv);
        for (int sweep = 0; sweep < CB_SWEEPS && na > 1; ++sweep) {
            double off = 0.0, dia = 0.0;
            for (int e = lane; e < CB_C * CB_C; e += 64) {
                const int i = e / CB_C, j = e % CB_C;
                const double v = B[e].x * B[e].x + B[e].y * B[e].y;
                if (i == j) dia += v; else off += 0.5 * v;
            }
            off = cb_wave_sum(off); dia = cb_wave_sum(dia);
            if (off <= a.jtol * dia || off == 0.0) break;
            for (int r = 0; r < Q; ++r) {
                if (lane < H) {
                    const int pi = xa < ya ? xa : ya, qi = xa < ya ? ya : xa;
                    advance(lane, xa, ya);
                    double c = 1.0;
                    cd se = make_double2(0.0, 0.0);
                    // Rotation angle in f32 with the hardware's 1-ulp rcp / rsq (no IEEE division sequences, no fp64
                    // Newton steps on 8 lanes), then (c, s) re-normalised in fp64 to second order: the rotation is
                    // unitary to 1e-21, it merely leaves ~1e-7 of the pivot behind, which the diagonal block below
                    // KEEPS and the next sweep removes.  (First order left every rotation 1e-14 off unitary: 2.6e-13
                    // of lambda_max after the ~100 rounds of a 16 x 16 problem.)
                    const cd bb = B[pi * CB_C + qi];
                    const float bx = (float)bb.x, by = (float)bb.y;
                    const float ab2 = bx * bx + by * by;
                    if (ab2 > 1e-37f) {
                        const float rab = __builtin_amdgcn_rsqf(ab2);                       // 1 / |b|
                        const float tau = 0.5f * (float)(B[qi * CB_C + qi].x - B[pi * CB_C + pi].x) * rab;
                        const float den = fabsf(tau) + __builtin_amdgcn_sqrtf(1.f + tau * tau);
                        const float t = __builtin_copysignf(__builtin_amdgcn_rcpf(den), tau);
                        const float cf = __builtin_amdgcn_rsqf(1.f + t * t);
                        const float sn = t * cf * rab;
                        const double cd0 = (double)cf, sx = (double)(sn * bx), sy = (double)(sn * by);
                        const double dl = (cd0 * cd0 + sx * sx + sy * sy) - 1.0;            // r = 1 + dl, dl = O(1e-7)
                        const double fix = 1.0 - 0.5 * dl + 0.375 * dl * dl;                // 1 / sqrt(r) + O(dl^3)
                        c = cd0 * fix;
                        se = make_double2(sx * fix, sy * fix);
                    }
                    rc[lane] = c; rs[lane] = se;
                }
                CB_WSYNC();
                const int up = xu < yu ? xu : yu, uq = xu < yu ? yu : xu, vp = xv < yv ? xv : yv, vq = xv < yv ? yv : xv;
                advance(bu, xu, yu);
                advance(bv, xv, yv);
                cd n00, n01, n10, n11;
                if (has_block) {
                    const double cu = rc[bu], cv = rc[bv];
                    const cd su = rs[bu], sv = rs[bv];
                    const cd b00 = B[up * CB_C + vp], b01 = B[up * CB_C + vq], b10 = B[uq * CB_C + vp], b11 = B[uq * CB_C + vq];
                    const cd svc = make_double2(sv.x, -sv.y), suc = make_double2(su.x, -su.y);
                    const cd a0 = zmul(svc, b01), a1 = zmul(sv, b00), a2 = zmul(svc, b11), a3 = zmul(sv, b10);
                    const cd t00 = make_double2(cv * b00.x - a0.x, cv * b00.y - a0.y);
                    const cd t01 = make_double2(a1.x + cv * b01.x, a1.y + cv * b01.y);
                    const cd t10 = make_double2(cv * b10.x - a2.x, cv * b10.y - a2.y);
                    const cd t11 = make_double2(a3.x + cv * b11.x, a3.y + cv * b11.y);
                    const cd c0 = zmul(su, t10), c1 = zmul(su, t11), c2 = zmul(suc, t00), c3 = zmul(suc, t01);
                    n00 = make_double2(cu * t00.x - c0.x, cu * t00.y - c0.y);
                    n01 = make_double2(cu * t01.x - c1.x, cu * t01.y - c1.y);
                    n10 = make_double2(c2.x + cu * t10.x, c2.y + cu * t10.y);
                    n11 = make_double2(c3.x + cu * t11.x, c3.y + cu * t11.y);
                }
                CB_WSYNC();                            // every block has read its inputs before anyone writes
                if (has_block) {
                    if (bu == bv) {
                        B[up * CB_C + up] = make_double2(n00.x, 0.0);
                        B[uq * CB_C + uq] = make_double2(n11.x, 0.0);
                        // (not 0: the angle is good to f32, and dropping the 1e-7 |pivot| it leaves is no similarity -- it moved
                        //  lambda_max by up to 1e-8 as long as the eigenvectors were dense, tests/test_gpu_canonical_values.py (h))
                        B[up * CB_C + uq] = n01;
                        B[uq * CB_C + up] = make_double2(n01.x, -n01.y);
                    } else {
                        B[up * CB_C + vp] = n00;
                        B[up * CB_C + vq] = n01;
                        B[uq * CB_C + vp] = n10;
                        B[uq * CB_C + vq] = n11;
                    }
                }
                CB_WSYNC();
            }
        }
        if (lane == 0) {
            double lmax = B[0].x;
            for (int q = 1; q < na; ++q) lmax = fmax(lmax, B[q * CB_C + q].x);
            if (!ok) { lmax = nan(""); atomicAdd(a.fail, 1); }
            double* o = a.out + bin * G * G;
            o[ga * G + gb] = lmax;
            o[gb * G + ga] = lmax;
        }
    }
}

// ---- the same pair problem without the Jacobi sweeps (round 5) ----------------------------------------------------------
// The parallel Jacobi above spends ~7 sweeps x 15 rounds x ~100 wave instructions per problem on ALL sixteen eigenvalues of
// B = M M^H (2.9 ms for the 61 560 problems of BASELINE configs[4]: fp64 issue-bound); only the largest one is asked for.
// Here B lives in REGISTERS (lane (i, jq) = row i, columns 4 jq .. 4 jq + 3: four complex entries), is reduced to a real symmetric
// tridiagonal matrix by fourteen Householder reflections (LAPACK zhetd2, lower form: p = tau B v, w = p - (tau / 2)(p^H v) v,
// B <- B - v w^H - w v^H; v and w travel through 512 bytes of LDS, sums over rows / column groups by lane shuffles), and the
// largest eigenvalue of T is bracketed by multisection on the Sturm sequence: 64 shifts per round, one per lane (x > lambda_max
// iff every leading principal minor of T - x changes sign), nine rounds from the Gershgorin bracket to the last bits.  Only |e_k|^2
// of the subdiagonal is needed, so a column that is already reduced needs no reflection.  LDS: M alone (4 KB a wave).
__device__ inline double cb_sum16(double v) {            // over the sixteen lanes of a row group, result in all of them
    for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ inline double cb_sum4(double v) {             // over the four row groups
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ inline double cb_lane(double v, int lane) {    // (lane: compile-time constant after unrolling)
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// largest eigenvalue of the Hermitian positive semi-definite 16 x 16 matrix held as a[c] = B[i][4 jq + c], i = lane & 15, jq = lane >> 4
// (rows / columns from the matrix order on: zero); vb: 32 complex numbers of this wave's LDS
__device__ double cb_top_eigenvalue(cd (&a)[4], cd* vb, int lane) {
    const int i = lane & 15, jq = lane >> 4;
    double d[16], e2[15];
#pragma unroll
    for (int k = 0; k < 14; ++k) {
        const int kq = k >> 2, src = 16 * kq;             // column k lives in row group kq, register k & 3
        const bool owner = jq == kq;
        const cd x = a[k & 3];
        d[k] = cb_lane(x.x, src + k);
        const double alr = cb_lane(x.x, src + k + 1), ali = cb_lane(x.y, src + k + 1);
        double s2 = (owner && i > k + 1) ? x.x * x.x + x.y * x.y : 0.0;
        s2 = cb_sum16(s2);
        const double xn2 = cb_lane(s2, src);
        e2[k] = alr * alr + ali * ali + xn2;
        if (xn2 == 0.0) continue;                         // (wave-uniform) nothing below the subdiagonal: no reflection
        const double beta = alr > 0.0 ? -sqrt(e2[k]) : sqrt(e2[k]), rb = 1.0 / beta;
        const cd tau = make_double2((beta - alr) * rb, -ali * rb);
        const double dr = alr - beta, den = 1.0 / (dr * dr + ali * ali);
        const cd sc = make_double2(dr * den, -ali * den);                       // 1 / (alpha - beta)
        if (owner) vb[i] = i > k + 1 ? zmul(x, sc) : (i == k + 1 ? make_double2(1.0, 0.0) : make_double2(0.0, 0.0));
        CB_WSYNC();
        const cd vi = vb[i];
        cd vc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) vc[c] = vb[4 * jq + c];
        cd acc = make_double2(0.0, 0.0);
#pragma unroll
        for (int c = 0; c < 4; ++c) { const cd t = zmul(a[c], vc[c]); acc.x += t.x; acc.y += t.y; }
        acc.x = cb_sum4(acc.x); acc.y = cb_sum4(acc.y);
        cd pv = zmul(tau, acc);
        if (i <= k) pv = make_double2(0.0, 0.0);
        const double kx = cb_sum16(pv.x * vi.x + pv.y * vi.y), ky = cb_sum16(pv.x * vi.y - pv.y * vi.x);      // p^H v
        const cd hk = zmul(make_double2(0.5 * tau.x, 0.5 * tau.y), make_double2(kx, ky));
        const cd t0 = zmul(hk, vi);
        const cd w = make_double2(pv.x - t0.x, pv.y - t0.y);
        if (jq == 0) vb[16 + i] = w;
        CB_WSYNC();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const cd wc = vb[16 + 4 * jq + c];
            const cd u0 = zmul_conj(vi, wc), u1 = zmul_conj(w, vc[c]);
            a[c].x -= u0.x + u1.x;
            a[c].y -= u0.y + u1.y;
        }
        CB_WSYNC();                                       // (v and w are read: the next step may write them)
    }
    d[14] = cb_lane(a[2].x, 48 + 14);
    d[15] = cb_lane(a[3].x, 48 + 15);
    {
        const double er = cb_lane(a[2].x, 48 + 15), ei = cb_lane(a[2].y, 48 + 15);
        e2[14] = er * er + ei * ei;
    }
    double dmax = d[0], emax = e2[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) dmax = fmax(dmax, d[q]);
#pragma unroll
    for (int q = 1; q < 15; ++q) emax = fmax(emax, e2[q]);
    const double top = dmax + 2.0 * sqrt(emax);           // Gershgorin; lambda_max >= the largest diagonal entry
    if (!(top > 0.0)) return dmax > 0.0 ? dmax : 0.0;
    const double sc1 = 1.0 / top, sc2 = sc1 * sc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) d[q] *= sc1;
#pragma unroll
    for (int q = 0; q < 15; ++q) e2[q] *= sc2;
    double lo = dmax * sc1, hi = 1.0;
    for (int round = 0; round < 9 && hi > lo; ++round) {
        const double x = lane == 63 ? hi : lo + (hi - lo) * ((double)(lane + 1) * (1.0 / 64.0));
        // x > lambda_max iff the leading principal minors p_q of T - x alternate in sign, p_q (-1)^q > 0.  The signs are compared, not
        // multiplied: with sixteen eigenvalues within 1e-11 of x the minors are ~1e-176 and the product of two consecutive ones is
        // below the smallest double -- `p2 * p1 < 0` then held for no lane and the loop left with the Gershgorin bracket still open
        // (rho_1^2 off by 1e4 x 2^-52, tests/test_gpu_canonical_values.py (d)).  A pair of minors that are both small is scaled up
        // (the recurrence is linear in (p0, p1): the signs stay), so the minors themselves cannot underflow either.
        double p0 = 1.0, p1 = d[0] - x;
        bool above = p1 < 0.0;
#pragma unroll
        for (int q = 1; q < 16; ++q) {
            double p2 = (d[q] - x) * p1 - e2[q - 1] * p0;
            above = above && ((q & 1) ? p2 > 0.0 : p2 < 0.0);
            if (fabs(p1) + fabs(p2) < 0x1p-400) { p1 *= 0x1p400; p2 *= 0x1p400; }
            p0 = p1; p1 = p2;
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(above);
        if (mask == 0ull) break;                          // (cannot happen for x = hi; rounding at the last bits)
        const int b = __builtin_ctzll(mask);
        const double xh = __shfl(x, b), xl = __shfl(x, b > 0 ? b - 1 : 0);
        hi = xh;
        if (b > 0) lo = xl;
    }
    return 0.5 * (lo + hi) * top;
}

template <bool IM>
__global__ void __launch_bounds__(64 * CB_WAVES) canonical_pair_hh_kernel(CanonArgs a, const cd* Lg, const int* okb) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int G = a.G;
    cd* scratch = reinterpret_cast<cd*>(cb_smem);                              // per wave: M, T [16][16]; v, w [32]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n_chunks = (a.n_gpairs + CB_WAVES - 1) / CB_WAVES;
    const int64_t bin = blockIdx.x / n_chunks;
    const int chunk = blockIdx.x % n_chunks;
    const ScRec rec = a.accum + bin * a.v.floats_per_bin;
    const cd* Ls = Lg + (size_t)bin * G * CB_C * CB_C;
    const int* okg = okb + bin * G;
    cd* M = scratch + (size_t)wave * (2 * CB_C * CB_C + 32);
    cd* T = M + CB_C * CB_C;
    cd* vb = T + CB_C * CB_C;
    const int pr = chunk * CB_WAVES + wave;
    if (pr >= a.n_gpairs) return;                                  // no workgroup barriers below
    int gp = pr, ga = 0, len = G - 1;
    while (gp >= len) { gp -= len; ++ga; --len; }
    const int gb = ga + 1 + gp;
    const int na = a.sizes[ga], nb = a.sizes[gb];
    const int32_t* ma = a.members + ga * CB_C;
    const int32_t* mb = a.members + gb * CB_C;
    const cd* La = Ls + (size_t)ga * CB_C * CB_C;
    const cd* Lb = Ls + (size_t)gb * CB_C * CB_C;
    const bool ok = okg[ga] && okg[gb];
    for (int e = lane; e < CB_C * CB_C; e += 64) {
        const int i = e / CB_C, j = e % CB_C;
        M[e] = (i < na && j < nb) ? csm_cross<IM>(rec, a, ma[i], mb[j]) : make_double2(0.0, 0.0);
    }
    CB_WSYNC();
    // M <- Linv_a M Linv_b^H as two dense products through T (the inverse factors come from the workspace: L2)
    for (int e = lane; e < CB_C * CB_C; e += 64) {
        const int i = e / CB_C, j = e % CB_C;
        cd la[CB_C];
#pragma unroll
        for (int k = 0; k < CB_C; ++k) la[k] = La[i * CB_C + k];
        cd sv = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < CB_C; ++k) { const cd t = zmul(la[k], M[k * CB_C + j]); sv.x += t.x; sv.y += t.y; }
        T[e] = sv;
    }
    CB_WSYNC();
    for (int e = lane; e < CB_C * CB_C; e += 64) {
        const int i = e / CB_C, j = e % CB_C;
        cd lb[CB_C];
#pragma unroll
        for (int k = 0; k < CB_C; ++k) lb[k] = Lb[j * CB_C + k];
        cd sv = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < CB_C; ++k) { const cd t = zmul_conj(T[i * CB_C + k], lb[k]); sv.x += t.x; sv.y += t.y; }
        M[e] = sv;
    }
    CB_WSYNC();
    // B = M M^H straight into the registers of the reduction: lane (i, jq) holds B[i][4 jq .. 4 jq + 3] (zero outside na x na)
    cd breg[4];
    {
        const int i = lane & 15, jq = lane >> 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * jq + c;
            cd sv = make_double2(0.0, 0.0);
            if (i < na && j < na) {
#pragma unroll
                for (int k = 0; k < CB_C; ++k) { const cd t = zmul_conj(M[i * CB_C + k], M[j * CB_C + k]); sv.x += t.x; sv.y += t.y; }
                if (i == j) sv.y = 0.0;
            }
            breg[c] = sv;
        }
    }
    double tr = 0.0;                                      // interaction view: trace(B), the diagonal of breg summed over the wave
    if constexpr (IM) {
        const int i = lane & 15, jq = lane >> 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) tr += (4 * jq + c == i) ? breg[c].x : 0.0;
        tr = cb_wave_sum(tr);
    }
    double lmax = cb_top_eigenvalue(breg, vb, lane);
    if (lane == 0) {
        if constexpr (IM) {
            if (!ok) atomicAdd(a.fail, 1);
            canon_store_interaction(a, bin, ga, gb, lmax, tr, ok);
        } else {
            if (!ok) { lmax = nan(""); atomicAdd(a.fail, 1); }
            double* o = a.out + bin * G * G;
            o[ga * G + gb] = lmax;
            o[gb * G + ga] = lmax;
        }
    }
}

// ---- groups of 33 ... 128 channels: a workgroup per (bin, group pair) -------------------------------------------------
// Three C x C matrices per problem no longer fit a lane's scratch (or the LDS): the group blocks S_aa, S_bb and the cross
// block S_ab of a problem live in a per-workgroup global scratch (L2-resident: 3 x 256 KB at 128 channels), factored and
// whitened by the workgroup's 256 threads in place -- right-looking Cholesky (one column per step), M <- L_a^-1 M with a
// thread per column, M <- M L_b^-H with a thread per row --, then B = M M^H goes into LDS as a packed upper triangle and
// the parallel cyclic Jacobi of the global-coherence kernel (sc_jacobi.h) diagonalises it: its largest diagonal entry
// is the squared canonical coherence.  Persistent workgroups (one per CU) walk the (bin, pair) list.
#define CBIG_C 128
#define CBIG_SWEEPS 14

__global__ void __launch_bounds__(256) canonical_big_kernel(CanonArgs a, cd* scratch, int64_t n_items) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    cd* B = reinterpret_cast<cd*>(cb_smem);                                  // packed upper triangle, <= 128 x 129 / 2
    constexpr int HM = CBIG_C / 2;
    double* rc = reinterpret_cast<double*>(B + (size_t)CBIG_C * (CBIG_C + 1) / 2);    // [HM]
    cd* rs = reinterpret_cast<cd*>(rc + HM);                                 // [HM]
    int* rp = reinterpret_cast<int*>(rs + HM);                               // [2 HM]
    unsigned short* blk_u = reinterpret_cast<unsigned short*>(rp + 2 * HM);  // [HM (HM + 1) / 2]
    unsigned short* blk_v = blk_u + HM * (HM + 1) / 2;
    __shared__ double red[2][256];
    __shared__ int done, n_rounds, bad, tab_for;
    const int tid = threadIdx.x;
    cd* La = scratch + (size_t)blockIdx.x * 3 * CBIG_C * CBIG_C;
    cd* Lb = La + CBIG_C * CBIG_C;
    cd* M = Lb + CBIG_C * CBIG_C;
    if (tid == 0) tab_for = -1;
    __syncthreads();
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t bin = item / a.n_gpairs;
        int gp = (int)(item - bin * a.n_gpairs);
        int ga = 0, len = a.G - 1;
        while (gp >= len) { gp -= len; ++ga; --len; }
        int gb = ga + 1 + gp;
        // the Jacobi runs on the SMALLER group's side: B = M M^H is n_a x n_a with the same non-zero spectrum either way
        if (a.sizes[gb] < a.sizes[ga]) { const int t = ga; ga = gb; gb = t; }
        const int na = a.sizes[ga], nb = a.sizes[gb];
        const int32_t* ma = a.members + ga * a.mstride;
        const int32_t* mb = a.members + gb * a.mstride;
        const ScRec rec = a.accum + bin * a.v.floats_per_bin;
        if (tid == 0) bad = 0;
        for (int e = tid; e < na * na; e += 256) { const int i = e / na, j = e % na; if (j <= i) La[i * CBIG_C + j] = csm_read(rec, a, ma[i], ma[j]); }
        for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, j = e % nb; if (j <= i) Lb[i * CBIG_C + j] = csm_read(rec, a, mb[i], mb[j]); }
        for (int e = tid; e < na * nb; e += 256) { const int i = e / nb, j = e % nb; M[i * CBIG_C + j] = csm_read(rec, a, ma[i], mb[j]); }
        __syncthreads();
        sc_wg_cholesky(La, CBIG_C, na, &bad);
        sc_wg_cholesky(Lb, CBIG_C, nb, &bad);
        // M <- La^-1 M: thread j owns column j (forward substitution down the rows)
        for (int j = tid; j < nb; j += 256)
            for (int i = 0; i < na; ++i) {
                cd sacc = M[i * CBIG_C + j];
                for (int k = 0; k < i; ++k) { const cd t = zmul(La[i * CBIG_C + k], M[k * CBIG_C + j]); sacc.x -= t.x; sacc.y -= t.y; }
                const double d = La[i * CBIG_C + i].x;
                M[i * CBIG_C + j] = make_double2(sacc.x / d, sacc.y / d);
            }
        __syncthreads();
        // M <- M Lb^-H: thread i owns row i (forward substitution along the columns)
        for (int i = tid; i < na; i += 256)
            for (int j = 0; j < nb; ++j) {
                cd sacc = M[i * CBIG_C + j];
                for (int k = 0; k < j; ++k) { const cd t = zmul_conj(M[i * CBIG_C + k], Lb[j * CBIG_C + k]); sacc.x -= t.x; sacc.y -= t.y; }
                const double d = Lb[j * CBIG_C + j].x;
                M[i * CBIG_C + j] = make_double2(sacc.x / d, sacc.y / d);
            }
        __syncthreads();
        // B = M M^H, packed upper triangle in LDS
        for (int e = tid; e < na * na; e += 256) {
            const int i = e / na, j = e % na;
            if (i > j) continue;
            cd sacc = make_double2(0.0, 0.0);
            for (int k = 0; k < nb; ++k) { const cd t = zmul_conj(M[i * CBIG_C + k], M[j * CBIG_C + k]); sacc.x += t.x; sacc.y += t.y; }
            if (i == j) sacc.y = 0.0;
            B[gc_tri(i, j, na)] = sacc;
        }
        const int H = (na + (na & 1)) / 2;
        if (tab_for != H) {                        // pairing table of this group size (rebuilt only when the size changes)
            __syncthreads();
            gc_block_table(blk_u, blk_v, H, tid);
            if (tid == 0) tab_for = H;
        }
        __syncthreads();
        gc_jacobi(B, na, rc, rs, rp, blk_u, blk_v, red, &done, &n_rounds, nullptr, CBIG_SWEEPS);
        __syncthreads();
        double lmax = -1.0;
        for (int i = tid; i < na; i += 256) lmax = fmax(lmax, B[gc_tri(i, i, na)].x);
        red[0][tid] = lmax;
        __syncthreads();
        for (int s2 = 128; s2 > 0; s2 >>= 1) {
            if (tid < s2) red[0][tid] = fmax(red[0][tid], red[0][tid + s2]);
            __syncthreads();
        }
        if (tid == 0) {
            double v = red[0][0];
            if (bad) { v = nan(""); atomicAdd(a.fail, 1); }
            double* o = a.out + bin * a.G * a.G;
            o[ga * a.G + gb] = v;
            o[gb * a.G + ga] = v;
        }
        __syncthreads();
    }
}

// ---- pieces the workgroup-per-pair kernels share (canonical_big_hh_kernel, interaction_vectors_kernel) ---------------------------
// item of the (bin, group pair) list that persistent workgroups walk -> its bin and its pair ga < gb (pairs in the row order of the
// upper triangle).  (The kernels above and canonical_big_hh_kernel keep these lines inline: calling this there costs the <false>
// instantiation an SGPR)
__device__ __forceinline__ void canon_item(const CanonArgs& a, int64_t item, int64_t& bin, int& ga, int& gb) {
    bin = item / a.n_gpairs;
    int gp = (int)(item - bin * a.n_gpairs);
    int len = a.G - 1;
    ga = 0;
    while (gp >= len) { gp -= len; ++ga; --len; }
    gb = ga + 1 + gp;
}
// The two whitening loops of a 256-thread workgroup on the na x nb block PM (row length ld, LDS or global), L Cholesky factors.
// M <- L_a^-1 M, right-looking: row k is final once it is divided by L_a[k][k]; every row below loses its multiple of it
__device__ __forceinline__ void canon_whiten_rows(cd* PA, cd* PM, int ld, int na, int nb, int tid) {
    for (int k = 0; k < na; ++k) {
        const double dk = PA[k * ld + k].x;
        if (tid < nb) { const cd v = PM[k * ld + tid]; PM[k * ld + tid] = make_double2(v.x / dk, v.y / dk); }
        __syncthreads();
        const int rows = na - k - 1;
        for (int e = tid; e < rows * nb; e += 256) {
            const int i = k + 1 + e / nb, j = e % nb;
            const cd t = zmul(PA[i * ld + k], PM[k * ld + j]);
            cd v = PM[i * ld + j];
            v.x -= t.x; v.y -= t.y;
            PM[i * ld + j] = v;
        }
        __syncthreads();
    }
}
// M <- M L_b^-H: column k is final once it is divided by L_b[k][k]; every column to its right loses conj(L_b[j][k]) times it
__device__ __forceinline__ void canon_whiten_cols(cd* PB, cd* PM, int ld, int na, int nb, int tid) {
    for (int k = 0; k < nb; ++k) {
        const double dk = PB[k * ld + k].x;
        if (tid < na) { const cd v = PM[tid * ld + k]; PM[tid * ld + k] = make_double2(v.x / dk, v.y / dk); }
        __syncthreads();
        const int cols = nb - k - 1;
        for (int e = tid; e < na * cols; e += 256) {
            const int i = e / cols, j = k + 1 + e % cols;
            const cd t = zmul_conj(PM[i * ld + k], PB[j * ld + k]);
            cd v = PM[i * ld + j];
            v.x -= t.x; v.y -= t.y;
            PM[i * ld + j] = v;
        }
        __syncthreads();
    }
}

// ---- the same problem with the largest eigenvalue alone (round 6) -------------------------------------------------------------
// canonical_big_kernel spends most of a problem in the parallel Jacobi (14 sweeps x (n - 1) rounds over the packed triangle:
// 2 ms of 3.6 at 64 channels, 21 ms a problem at 128) for ONE number, the largest eigenvalue of B = M M^H.  Here B is reduced
// to a real symmetric tridiagonal matrix by n - 2 Householder reflections (LAPACK zhetd2, lower form, one thread per row of the
// trailing block: p = tau B22 v, w = p - (tau / 2)(p^H v) v, B22 <- B22 - v w^H - w v^H; only the diagonal and the SQUARES of the
// subdiagonal are kept, no reflector is stored), and lambda_max is bracketed by multisection on the Sturm count: 256 shifts a
// round, one per thread, seven rounds from the Gershgorin bracket to the last bits.  B (full storage, column-major) lives in
// LDS up to 96 channels, beyond in the workgroup's global scratch (the block La is free once M is whitened).
#define CBH_LDS_N 96
#define CBH_SMALL 64           // pairs of groups of at most this many channels are processed in LDS entirely
#define CBH_LD 65              // their row length (odd: a column walk touches every bank)
template <bool IM>
__global__ void __launch_bounds__(256) canonical_big_hh_kernel(CanonArgs a, cd* scratch, int64_t n_items, int small_n, int small_ld) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    cd* Bl = reinterpret_cast<cd*>(cb_smem);                 // CBH_LDS_N^2 elements: B (column-major) or, for pairs of groups of at
    __shared__ double dg[CBIG_C], e2[CBIG_C];                // most CBH_SMALL channels, the whole problem (one factor block + M)
    __shared__ cd vs[CBIG_C], ws[CBIG_C];
    __shared__ double red4[4], sh[2];
    __shared__ int bad, first_above;
    const int tid = threadIdx.x;
    // (scratch == nullptr: every pair of this launch fits LDS -- small_n is the largest group -- and the three pointers are never used)
    cd* Lag = scratch ? scratch + (size_t)blockIdx.x * 3 * CBIG_C * CBIG_C : nullptr;
    cd* Lbg = scratch ? Lag + CBIG_C * CBIG_C : nullptr;
    cd* Mg = scratch ? Lbg + CBIG_C * CBIG_C : nullptr;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t bin = item / a.n_gpairs;
        int gp = (int)(item - bin * a.n_gpairs);
        int ga = 0, len = a.G - 1;
        while (gp >= len) { gp -= len; ++ga; --len; }
        int gb = ga + 1 + gp;
        if (a.sizes[gb] < a.sizes[ga]) { const int t = ga; ga = gb; gb = t; }      // B on the smaller group's side
        const int na = a.sizes[ga], nb = a.sizes[gb];
        const int32_t* ma = a.members + ga * a.mstride;
        const int32_t* mb = a.members + gb * a.mstride;
        const ScRec rec = a.accum + bin * a.v.floats_per_bin;
        // Pairs of groups of at most CBH_SMALL channels stay in LDS from the records to lambda_max: one factor block at a time (L_b takes
        // L_a's place once M is multiplied by L_a^-1, B takes L_b's) beside M; larger pairs keep the three blocks in the global scratch.
        // (small_n: CBH_SMALL, or the largest group when no group is larger -- the launch then asks for 2 small_n small_ld elements of LDS
        //  only and several workgroups share a compute unit: 34 KB at 32 channels)
        const bool small = nb <= small_n;                    // (na <= nb)
        cd* PA = small ? Bl : Lag;
        cd* PB = small ? Bl : Lbg;
        cd* PM = small ? Bl + small_n * small_ld : Mg;
        const int ld = small ? small_ld : CBIG_C;
        if (tid == 0) bad = 0;
        for (int e = tid; e < na * na; e += 256) { const int i = e / na, j = e % na; if (j <= i) PA[i * ld + j] = csm_group<IM>(rec, a, ma[i], ma[j]); }
        for (int e = tid; e < na * nb; e += 256) { const int i = e / nb, j = e % nb; PM[i * ld + j] = csm_cross<IM>(rec, a, ma[i], mb[j]); }
        __syncthreads();
        sc_wg_cholesky(PA, ld, na, &bad);
        canon_whiten_rows(PA, PM, ld, na, nb, tid);
        for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, j = e % nb; if (j <= i) PB[i * ld + j] = csm_group<IM>(rec, a, mb[i], mb[j]); }
        __syncthreads();
        sc_wg_cholesky(PB, ld, nb, &bad);
        canon_whiten_cols(PB, PM, ld, na, nb, tid);
        // B = M M^H, full storage, column-major with leading dimension na (small pairs: where the factor blocks were)
        cd* B = (small || na <= CBH_LDS_N) ? Bl : Lag;
        for (int e = tid; e < na * na; e += 256) {
            const int i = e % na, j = e / na;
            cd sacc = make_double2(0.0, 0.0);
            for (int k = 0; k < nb; ++k) { const cd t = zmul_conj(PM[i * ld + k], PM[j * ld + k]); sacc.x += t.x; sacc.y += t.y; }
            if (i == j) sacc.y = 0.0;
            B[(size_t)j * na + i] = sacc;
        }
        __syncthreads();
        // ---- tridiagonalisation (zhetd2, lower): d, e^2 ----
        for (int k = 0; k + 1 < na; ++k) {
            const int m = na - k - 1;                        // order of the trailing block
            const cd* col = B + (size_t)k * na + (k + 1);
            cd xi = make_double2(0.0, 0.0);
            if (tid < m) xi = col[tid];
            if (tid == 0) { sh[0] = xi.x; sh[1] = xi.y; dg[k] = B[(size_t)k * na + k].x; }
            const double xn2 = sc_wg_sum((tid >= 1 && tid < m) ? xi.x * xi.x + xi.y * xi.y : 0.0, red4, tid);
            const double alr = sh[0], ali = sh[1];
            if (xn2 == 0.0 && ali == 0.0) {                  // H = I (uniform over the workgroup)
                if (tid == 0) e2[k] = alr * alr;
                __syncthreads();
                continue;
            }
            const double nrm = sqrt(alr * alr + ali * ali + xn2);
            const double beta = alr >= 0.0 ? -nrm : nrm;
            const cd tk = make_double2((beta - alr) / beta, -ali / beta);
            cd vi = make_double2(0.0, 0.0);
            {
                const double dr = alr - beta, di = ali, dd = dr * dr + di * di;
                const cd scale = make_double2(dr / dd, -di / dd);          // 1 / (alpha - beta)
                if (tid < m) { vi = tid == 0 ? make_double2(1.0, 0.0) : zmul(xi, scale); vs[tid] = vi; }
                if (tid == 0) e2[k] = beta * beta;
            }
            __syncthreads();
            const cd* B22 = B + (size_t)(k + 1) * na + (k + 1);
            cd pi = make_double2(0.0, 0.0);
            if (tid < m) {
                cd acc = make_double2(0.0, 0.0);
                for (int j = 0; j < m; ++j) {
                    const cd aij = B22[(size_t)j * na + tid], vj = vs[j];
                    acc.x += aij.x * vj.x - aij.y * vj.y;
                    acc.y += aij.x * vj.y + aij.y * vj.x;
                }
                pi = zmul(tk, acc);
            }
            const double dre = sc_wg_sum(pi.x * vi.x + pi.y * vi.y, red4, tid);       // p^H v
            const double dim = sc_wg_sum(pi.x * vi.y - pi.y * vi.x, red4, tid);
            const cd al2 = zmul(make_double2(-0.5 * tk.x, -0.5 * tk.y), make_double2(dre, dim));
            cd wi = make_double2(0.0, 0.0);
            if (tid < m) {
                const cd t = zmul(al2, vi);
                wi = make_double2(pi.x + t.x, pi.y + t.y);
                ws[tid] = wi;
            }
            __syncthreads();
            if (tid < m) {
                cd* row = B + (size_t)(k + 1) * na + (k + 1) + tid;
                for (int j = 0; j < m; ++j) {
                    const cd wj = ws[j], vj = vs[j];
                    cd aij = row[(size_t)j * na];
                    aij.x -= vi.x * wj.x + vi.y * wj.y + wi.x * vj.x + wi.y * vj.y;       // a_ij -= v_i conj(w_j) + w_i conj(v_j)
                    aij.y -= vi.y * wj.x - vi.x * wj.y + wi.y * vj.x - wi.x * vj.y;
                    row[(size_t)j * na] = aij;
                }
            }
            __syncthreads();
        }
        if (tid == 0) { dg[na - 1] = B[(size_t)(na - 1) * na + (na - 1)].x; e2[na - 1] = 0.0; }
        __syncthreads();
        // ---- lambda_max by multisection on the Sturm count (x > lambda_max iff all n leading minors of T - x are negative) ----
        double lo, hi;
        {
            double g_hi = -1e300, g_lo = 1e300, emax = 0.0;
            for (int i = 0; i < na; ++i) {                   // (every thread: n <= 128 LDS reads)
                const double el = i > 0 ? sqrt(e2[i - 1]) : 0.0, er = i + 1 < na ? sqrt(e2[i]) : 0.0;
                g_hi = fmax(g_hi, dg[i] + el + er); g_lo = fmin(g_lo, dg[i] - el - er);
                emax = fmax(emax, e2[i]);
            }
            const double tn = fmax(fabs(g_hi), fabs(g_lo));
            const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax);
            const double pad = 2.0 * tn * 2.220446049250313e-16 * na + 2.0 * pivmin;
            lo = g_lo - pad; hi = g_hi + pad;
            for (int round = 0; round < 8; ++round) {
                const double x = lo + (hi - lo) * ((double)(tid + 1) / 257.0);
                int cnt = 0;
                double q = dg[0] - x;
                if (fabs(q) < pivmin) q = -pivmin;
                cnt += q < 0.0;
                for (int i = 1; i < na; ++i) {
                    q = dg[i] - x - e2[i - 1] / q;
                    if (fabs(q) < pivmin) q = -pivmin;
                    cnt += q < 0.0;
                }
                if (tid == 0) first_above = 256;
                __syncthreads();
                if (cnt == na) atomicMin(&first_above, tid);     // every eigenvalue lies below x
                __syncthreads();
                const int f = first_above;
                const double nlo = f == 0 ? lo : lo + (hi - lo) * ((double)f / 257.0);
                const double nhi = f == 256 ? hi : lo + (hi - lo) * ((double)(f + 1) / 257.0);
                __syncthreads();
                if (!(nhi - nlo < hi - lo)) break;           // (uniform: the bracket is down to neighbouring doubles)
                lo = nlo; hi = nhi;
            }
        }
        if (tid == 0) {
            double v = fmax(0.5 * (lo + hi), 0.0);            // (B = 0: the last bracket is +- pivmin around 0, B >= 0: never below)
            if constexpr (IM) {
                double tr = 0.0;                             // trace(B) = trace(T): the reflections are unitary similarities
                for (int i = 0; i < na; ++i) tr += dg[i];
                if (bad) atomicAdd(a.fail, 1);
                canon_store_interaction(a, bin, ga, gb, v, tr, !bad);
            } else {
                if (bad) { v = nan(""); atomicAdd(a.fail, 1); }
                double* o = a.out + bin * a.G * a.G;
                o[ga * a.G + gb] = v;
                o[gb * a.G + ga] = v;
            }
        }
        __syncthreads();
    }
}

// ---- the vectors that attain MIC -----------------------------------------------------------------------------
// With R_g = Re S_gg = L_g L_g^T, I = Im S_ab and M = L_a^-1 I L_b^-T (the interaction view holds it as (0, M): every product
// below reads the imaginary parts), p the unit eigenvector of B = M M^T for lambda_max = MIC^2 and q = M^T p / MIC:
//     filters   alpha = L_a^-T p,  beta = L_b^-T q        patterns   a = L_a p,  b = L_b q.
// The kernels above drop what the vectors are made of (no reflector is stored, B takes the place of the factor blocks), so this
// one keeps L_a, L_b and M of a pair until the back-substitutions -- in LDS while the pair fits beside B (both groups of at most
// `lds_n` channels: iv_lds_n), else in the workgroup's global scratch -- and diagonalises B (packed triangle in LDS) with the
// parallel Jacobi of sc_jacobi.h, whose rotation log gives p = J_1 ... J_m e_k as global_coherence_big_kernel recovers its
// vectors.  B is real in this view, so every rotation is real (Im s = 0 exactly) and the back-application is real arithmetic.
// B sits on the smaller group's side; when that is the group with the higher label the cross block read is Im S_ba = -I^T and
// the second vector changes sign with it.  One joint sign: the largest entry (lowest index on a tie) of the pattern of the
// group with the lower label is positive.
#define IV_SWEEPS CBIG_SWEEPS
#define IV_STATIC_LDS 6144                     // reserve for the kernel's static LDS (red and a few scalars: 4144 bytes)
#define IV_LDS_LIMIT (160 * 1024)

struct IvArgs {
    double* filters;       // [n_bins][G][G][vstride]
    double* patterns;
    double* log;           // [slots][IV_SWEEPS (Mb - 1)][Hb][3] rotation log, Mb = max group size rounded up to even, Hb = Mb / 2
    cd* scratch;           // [slots][3][CBIG_C][CBIG_C] or NULL when every pair fits LDS
    int vstride;           // = max group size
    int bn;                // largest order of B the LDS layout holds (= max group size)
    int lds_n, lds_ld;     // pairs of groups of at most lds_n channels stay in LDS; their row length
};

// dynamic LDS of a launch: the packed triangle of B and the Jacobi's tables for groups of up to bn channels, four vectors, and
// three blocks of lds_n x (lds_n | 1)
// (vec: the size of a vector entry -- double here, cd for the canonical vectors below)
static size_t iv_lds_bytes(int bn, int lds_n, size_t vec = sizeof(double)) {
    const size_t hm = (size_t)(bn + 1) / 2;
    return ((size_t)bn * (bn + 1) / 2 + hm + (size_t)3 * lds_n * (lds_n | 1)) * sizeof(cd) + 4 * CBIG_C * vec + hm * sizeof(double) +
           2 * hm * sizeof(int) + hm * (hm + 1) * sizeof(unsigned short) + 16;
}
// the largest group size up to which a pair keeps its blocks in LDS, in a launch whose largest group has max_group channels
static int iv_lds_n(int max_group, size_t vec = sizeof(double)) {
    int n = max_group;
    while (n > 0 && iv_lds_bytes(max_group, n, vec) + IV_STATIC_LDS > IV_LDS_LIMIT) --n;
    return n;
}
extern "C" int sc_interaction_vectors_lds_group(int max_group_size) {
    return max_group_size < 1 || max_group_size > CBIG_C ? 0 : iv_lds_n(max_group_size);
}

// x <- L^-T x for the two groups at once (threads 0 .. 127: group a, 128 .. 255: group b), column-oriented back-substitution
__device__ inline void iv_back_substitute(const cd* La, const cd* Lb, int lda, int ldb, int na, int nb, double* xa, double* xb, int tid) {
    const int nmax = na > nb ? na : nb;
    for (int i = nmax - 1; i >= 0; --i) {
        if (tid == 0 && i < na) xa[i] /= La[i * lda + i].x;
        if (tid == 128 && i < nb) xb[i] /= Lb[i * ldb + i].x;
        __syncthreads();
        if (tid < 128) { if (i < na && tid < i) xa[tid] -= La[i * lda + tid].x * xa[i]; }
        else { const int k = tid - 128; if (i < nb && k < i) xb[k] -= Lb[i * ldb + k].x * xb[i]; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) interaction_vectors_kernel(CanonArgs a, IvArgs v, int64_t n_items) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int hm = (v.bn + 1) / 2;
    cd* B = reinterpret_cast<cd*>(cb_smem);                                    // packed upper triangle, bn (bn + 1) / 2
    cd* rs = B + (size_t)v.bn * (v.bn + 1) / 2;                                // [hm]
    cd* blocks = rs + hm;                                                      // [3][lds_n][lds_ld]
    double* pv = reinterpret_cast<double*>(blocks + (size_t)3 * v.lds_n * v.lds_ld);   // [CBIG_C] p, then the pattern of a
    double* qv = pv + CBIG_C;                                                  // q, then the pattern of b
    double* xa = qv + CBIG_C;                                                  // the filter of a
    double* xb = xa + CBIG_C;                                                  // the filter of b
    double* rc = xb + CBIG_C;                                                  // [hm]
    int* rp = reinterpret_cast<int*>(rc + hm);                                 // [2 hm]
    unsigned short* blk_u = reinterpret_cast<unsigned short*>(rp + 2 * hm);    // [hm (hm + 1) / 2]
    unsigned short* blk_v = blk_u + hm * (hm + 1) / 2;
    __shared__ double red[2][256];
    __shared__ double sh_lmax, sh_tr, sh_sign;
    __shared__ int done, n_rounds, bad, tab_for, sh_src;
    const int tid = threadIdx.x;
    cd* Lag = v.scratch ? v.scratch + (size_t)blockIdx.x * 3 * CBIG_C * CBIG_C : nullptr;
    const int Mb = v.bn + (v.bn & 1);
    double* mylog = v.log + (size_t)blockIdx.x * IV_SWEEPS * (Mb - 1) * (Mb / 2) * 3;
    if (tid == 0) tab_for = -1;
    __syncthreads();
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        int64_t bin;
        int g_lo, g_hi;
        canon_item(a, item, bin, g_lo, g_hi);
        // B on the smaller group's side: ga is that group.  flip: the cross block read below is then Im S_ba = -(Im S_ab)^T
        const bool flip = a.sizes[g_hi] < a.sizes[g_lo];
        const int ga = flip ? g_hi : g_lo, gb = flip ? g_lo : g_hi;
        const int na = a.sizes[ga], nb = a.sizes[gb];
        const int32_t* ma = a.members + ga * a.mstride;
        const int32_t* mb = a.members + gb * a.mstride;
        const ScRec rec = a.accum + bin * a.v.floats_per_bin;
        const bool in_lds = nb <= v.lds_n;                   // (na <= nb)
        const int ld = in_lds ? v.lds_ld : CBIG_C;
        cd* PA = in_lds ? blocks : Lag;
        cd* PB = PA + (in_lds ? v.lds_n * v.lds_ld : CBIG_C * CBIG_C);
        cd* PM = PB + (in_lds ? v.lds_n * v.lds_ld : CBIG_C * CBIG_C);
        if (tid == 0) bad = 0;
        for (int e = tid; e < na * na; e += 256) { const int i = e / na, j = e % na; if (j <= i) PA[i * ld + j] = csm_group<true>(rec, a, ma[i], ma[j]); }
        for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, j = e % nb; if (j <= i) PB[i * ld + j] = csm_group<true>(rec, a, mb[i], mb[j]); }
        for (int e = tid; e < na * nb; e += 256) { const int i = e / nb, j = e % nb; PM[i * ld + j] = csm_cross<true>(rec, a, ma[i], mb[j]); }
        __syncthreads();
        sc_wg_cholesky(PA, ld, na, &bad);
        sc_wg_cholesky(PB, ld, nb, &bad);
        canon_whiten_rows(PA, PM, ld, na, nb, tid);
        canon_whiten_cols(PB, PM, ld, na, nb, tid);
        // B = M M^H (real: M is (0, m)), packed upper triangle in LDS
        for (int e = tid; e < na * na; e += 256) {
            const int i = e / na, j = e % na;
            if (i > j) continue;
            double sacc = 0.0;
            for (int k = 0; k < nb; ++k) sacc += PM[i * ld + k].y * PM[j * ld + k].y;
            B[gc_tri(i, j, na)] = make_double2(sacc, 0.0);
        }
        const int H = (na + (na & 1)) / 2;
        if (tab_for != H) {                        // pairing table of this group size (rebuilt only when the size changes)
            __syncthreads();
            gc_block_table(blk_u, blk_v, H, tid);
            if (tid == 0) tab_for = H;
        }
        __syncthreads();
        if (tid == 0) {                            // trace(B) = MIM before the rotations: the clamp of canon_store_interaction
            double tr = 0.0;
            for (int i = 0; i < na; ++i) tr += B[gc_tri(i, i, na)].x;
            sh_tr = tr;
        }
        gc_jacobi(B, na, rc, rs, rp, blk_u, blk_v, red, &done, &n_rounds, mylog, IV_SWEEPS);
        __syncthreads();
        if (tid == 0) {
            int src = 0;
            double lmax = B[0].x;
            for (int i = 1; i < na; ++i) { const double d = B[gc_tri(i, i, na)].x; if (d > lmax) { lmax = d; src = i; } }
            sh_src = src; sh_lmax = lmax;
        }
        __syncthreads();
        // p = J_1 ... J_m e_src, right to left; thread t rotates the entries of pair t of the round
        for (int i = tid; i < na; i += 256) pv[i] = i == sh_src ? 1.0 : 0.0;
        __syncthreads();
        {
            const int Mp = na + (na & 1);
            const int total_rounds = n_rounds;
            for (int rr = total_rounds - 1; rr >= 0; --rr) {
                const int r = rr % (Mp - 1);
                if (tid < H) {
                    int x, y;
                    if (tid == 0) { x = Mp - 1; y = r; }
                    else { x = (r + tid) % (Mp - 1); y = (r - tid + (Mp - 1)) % (Mp - 1); }
                    const int pi = x < y ? x : y, qi = x < y ? y : x;
                    if (qi < na) {
                        const double* lg = mylog + ((size_t)rr * H + tid) * 3;
                        const double c = lg[0], s = lg[1];
                        const double xp = pv[pi], xq = pv[qi];
                        pv[pi] = c * xp + s * xq;
                        pv[qi] = c * xq - s * xp;
                    }
                }
                __syncthreads();
            }
        }
        const double tr = sh_tr;
        const double mic = sqrt(fmin(fmax(sh_lmax, 0.0), tr));
        const bool defined = !bad && tr > 0.0 && mic > 0.0;                   // (B = 0 exactly: MIC 0, no vectors)
        // q = +-M^T p / MIC, the filters' right-hand sides, then the patterns L p, L q in place of p, q
        for (int j = tid; j < nb; j += 256) {
            double sacc = 0.0;
            for (int i = 0; i < na; ++i) sacc += PM[i * ld + j].y * pv[i];
            const double qj = (flip ? -sacc : sacc) / mic;
            qv[j] = qj; xb[j] = qj;
        }
        for (int i = tid; i < na; i += 256) xa[i] = pv[i];
        __syncthreads();
        double pat = 0.0;
        if (tid < 128) { if (tid < na) for (int k = 0; k <= tid; ++k) pat += PA[tid * ld + k].x * pv[k]; }
        else { const int j = tid - 128; if (j < nb) for (int k = 0; k <= j; ++k) pat += PB[j * ld + k].x * qv[k]; }
        __syncthreads();
        if (tid < 128) { if (tid < na) pv[tid] = pat; }
        else if (tid - 128 < nb) qv[tid - 128] = pat;
        iv_back_substitute(PA, PB, ld, ld, na, nb, xa, xb, tid);
        if (tid == 0) {
            const double* lowp = flip ? qv : pv;             // the pattern of the group with the lower label
            const int nl = flip ? nb : na;
            double best = -1.0, val = 1.0;
            for (int i = 0; i < nl; ++i) { const double m = fabs(lowp[i]); if (m > best) { best = m; val = lowp[i]; } }
            sh_sign = val < 0.0 ? -1.0 : 1.0;
            double* o = a.out + bin * a.G * a.G;
            const double m = bad ? nan("") : mic;
            o[ga * a.G + gb] = m;
            o[gb * a.G + ga] = m;
            if (bad) atomicAdd(a.fail, 1);
        }
        __syncthreads();
        if (defined) {                                       // (the outputs are NaN-filled before the launch)
            const double sg = sh_sign;
            const size_t oa = (((size_t)bin * a.G + ga) * a.G + gb) * v.vstride, ob = (((size_t)bin * a.G + gb) * a.G + ga) * v.vstride;
            for (int i = tid; i < na; i += 256) { v.filters[oa + i] = sg * xa[i]; v.patterns[oa + i] = sg * pv[i]; }
            for (int j = tid; j < nb; j += 256) { v.filters[ob + j] = sg * xb[j]; v.patterns[ob + j] = sg * qv[j]; }
        }
        __syncthreads();
    }
}

// ---- the vectors that attain canonical coherence, and its whole spectrum ----------------------------------------
// The complex-Hermitian sibling of interaction_vectors_kernel, on the records as canonical coherence reads them (csm_group<false>,
// csm_cross<false>): S_gg = L_g L_g^H, M = L_a^-1 S_ab L_b^-H, B = M M^H (packed Hermitian triangle in LDS) with eigenvalues
// rho_1^2 >= rho_2^2 >= ..., p the unit eigenvector for rho_1^2 -- from the complex rotation log, J = [[c, s], [-conj s, c]] -- and
// q = M^H p / rho_1:
//     filters   alpha = L_a^-H p,  beta = L_b^-H q        patterns   a = L_a p,  b = L_b q        coherences  rho_k, descending.
// Same residency rule, workspace and item walk as the kernel above; the four vectors are complex, so the LDS edge is
// iv_lds_n(n, sizeof(cd)).  When B sits on the side of the group with the higher label the cross block read is S_ba = S_ab^H: M
// becomes M^H and p, q change roles -- no sign changes.  One joint unit phase: the entry of largest magnitude (lowest index on a
// tie) of the pattern of the group with the lower label is real and positive (global_coherence's rule).
struct CvArgs {
    double* coherences;    // [n_bins][G][G][vstride]
    cd* filters;           // [n_bins][G][G][vstride]
    cd* patterns;
    double* log;           // as IvArgs
    cd* scratch;
    int vstride, bn, lds_n, lds_ld;
};

extern "C" int sc_canonical_vectors_lds_group(int max_group_size) {
    return max_group_size < 1 || max_group_size > CBIG_C ? 0 : iv_lds_n(max_group_size, sizeof(cd));
}

// x <- L^-H x for the two groups at once (threads 0 .. 127: group a, 128 .. 255: group b), column-oriented back-substitution
__device__ inline void cv_back_substitute(const cd* La, const cd* Lb, int lda, int ldb, int na, int nb, cd* xa, cd* xb, int tid) {
    const int nmax = na > nb ? na : nb;
    for (int i = nmax - 1; i >= 0; --i) {
        if (tid == 0 && i < na) { const double d = La[i * lda + i].x; xa[i] = make_double2(xa[i].x / d, xa[i].y / d); }
        if (tid == 128 && i < nb) { const double d = Lb[i * ldb + i].x; xb[i] = make_double2(xb[i].x / d, xb[i].y / d); }
        __syncthreads();
        if (tid < 128) {
            if (i < na && tid < i) { const cd t = zmul_conj(xa[i], La[i * lda + tid]); xa[tid].x -= t.x; xa[tid].y -= t.y; }
        } else {
            const int k = tid - 128;
            if (i < nb && k < i) { const cd t = zmul_conj(xb[i], Lb[i * ldb + k]); xb[k].x -= t.x; xb[k].y -= t.y; }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) canonical_vectors_kernel(CanonArgs a, CvArgs v, int64_t n_items) {
    extern __shared__ __align__(16) unsigned char cb_smem[];
    const int hm = (v.bn + 1) / 2;
    cd* B = reinterpret_cast<cd*>(cb_smem);                                    // packed upper triangle, bn (bn + 1) / 2
    cd* rs = B + (size_t)v.bn * (v.bn + 1) / 2;                                // [hm]
    cd* blocks = rs + hm;                                                      // [3][lds_n][lds_ld]
    cd* pv = blocks + (size_t)3 * v.lds_n * v.lds_ld;                          // [CBIG_C] p, then the pattern of a
    cd* qv = pv + CBIG_C;                                                      // q, then the pattern of b
    cd* xa = qv + CBIG_C;                                                      // the filter of a
    cd* xb = xa + CBIG_C;                                                      // the filter of b
    double* rc = reinterpret_cast<double*>(xb + CBIG_C);                       // [hm]
    int* rp = reinterpret_cast<int*>(rc + hm);                                 // [2 hm]
    unsigned short* blk_u = reinterpret_cast<unsigned short*>(rp + 2 * hm);    // [hm (hm + 1) / 2]
    unsigned short* blk_v = blk_u + hm * (hm + 1) / 2;
    __shared__ double red[2][256];                           // the Jacobi's reduction; then the eigenvalues and their sorted copy
    __shared__ double sh_tr;
    __shared__ cd sh_phase;
    __shared__ int done, n_rounds, bad, tab_for, sh_src;
    const int tid = threadIdx.x;
    cd* Lag = v.scratch ? v.scratch + (size_t)blockIdx.x * 3 * CBIG_C * CBIG_C : nullptr;
    const int Mb = v.bn + (v.bn & 1);
    double* mylog = v.log + (size_t)blockIdx.x * IV_SWEEPS * (Mb - 1) * (Mb / 2) * 3;
    if (tid == 0) tab_for = -1;
    __syncthreads();
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        int64_t bin;
        int g_lo, g_hi;
        canon_item(a, item, bin, g_lo, g_hi);
        // B on the smaller group's side: ga is that group.  flip: the cross block read below is then S_ba = S_ab^H
        const bool flip = a.sizes[g_hi] < a.sizes[g_lo];
        const int ga = flip ? g_hi : g_lo, gb = flip ? g_lo : g_hi;
        const int na = a.sizes[ga], nb = a.sizes[gb];
        const int32_t* ma = a.members + ga * a.mstride;
        const int32_t* mb = a.members + gb * a.mstride;
        const ScRec rec = a.accum + bin * a.v.floats_per_bin;
        const bool in_lds = nb <= v.lds_n;                   // (na <= nb)
        const int ld = in_lds ? v.lds_ld : CBIG_C;
        cd* PA = in_lds ? blocks : Lag;
        cd* PB = PA + (in_lds ? v.lds_n * v.lds_ld : CBIG_C * CBIG_C);
        cd* PM = PB + (in_lds ? v.lds_n * v.lds_ld : CBIG_C * CBIG_C);
        if (tid == 0) bad = 0;
        for (int e = tid; e < na * na; e += 256) { const int i = e / na, j = e % na; if (j <= i) PA[i * ld + j] = csm_group<false>(rec, a, ma[i], ma[j]); }
        for (int e = tid; e < nb * nb; e += 256) { const int i = e / nb, j = e % nb; if (j <= i) PB[i * ld + j] = csm_group<false>(rec, a, mb[i], mb[j]); }
        for (int e = tid; e < na * nb; e += 256) { const int i = e / nb, j = e % nb; PM[i * ld + j] = csm_cross<false>(rec, a, ma[i], mb[j]); }
        __syncthreads();
        sc_wg_cholesky(PA, ld, na, &bad);
        sc_wg_cholesky(PB, ld, nb, &bad);
        canon_whiten_rows(PA, PM, ld, na, nb, tid);
        canon_whiten_cols(PB, PM, ld, na, nb, tid);
        // B = M M^H, packed upper triangle in LDS (the diagonal exactly real)
        for (int e = tid; e < na * na; e += 256) {
            const int i = e / na, j = e % na;
            if (i > j) continue;
            cd sacc = make_double2(0.0, 0.0);
            for (int k = 0; k < nb; ++k) { const cd t = zmul_conj(PM[i * ld + k], PM[j * ld + k]); sacc.x += t.x; sacc.y += t.y; }
            if (i == j) sacc.y = 0.0;
            B[gc_tri(i, j, na)] = sacc;
        }
        const int H = (na + (na & 1)) / 2;
        if (tab_for != H) {                        // pairing table of this group size (rebuilt only when the size changes)
            __syncthreads();
            gc_block_table(blk_u, blk_v, H, tid);
            if (tid == 0) tab_for = H;
        }
        __syncthreads();
        if (tid == 0) {                            // trace(B) before the rotations: exactly 0 only where the cross block is 0
            double tr = 0.0;
            for (int i = 0; i < na; ++i) tr += B[gc_tri(i, i, na)].x;
            sh_tr = tr;
        }
        gc_jacobi(B, na, rc, rs, rp, blk_u, blk_v, red, &done, &n_rounds, mylog, IV_SWEEPS);
        __syncthreads();
        // the spectrum in descending order by rank counting (equal values: the lower index first); rank 0 names the eigenvector
        if (tid < na) red[0][tid] = B[gc_tri(tid, tid, na)].x;
        __syncthreads();
        if (tid < na) {
            const double mine = red[0][tid];
            int rank = 0;
            for (int j = 0; j < na; ++j) { const double o = red[0][j]; rank += (o > mine || (o == mine && j < tid)) ? 1 : 0; }
            if (rank < na) red[1][rank] = mine;    // (NaN eigenvalues of a failed block all count 0: such a pair stays NaN below)
            if (rank == 0) sh_src = tid;
        }
        __syncthreads();
        // p = J_1 ... J_m e_src, right to left; thread t rotates the entries of pair t of the round
        for (int i = tid; i < na; i += 256) pv[i] = make_double2(i == sh_src ? 1.0 : 0.0, 0.0);
        __syncthreads();
        {
            const int Mp = na + (na & 1);
            const int total_rounds = n_rounds;
            for (int rr = total_rounds - 1; rr >= 0; --rr) {
                const int r = rr % (Mp - 1);
                if (tid < H) {
                    int x, y;
                    if (tid == 0) { x = Mp - 1; y = r; }
                    else { x = (r + tid) % (Mp - 1); y = (r - tid + (Mp - 1)) % (Mp - 1); }
                    const int pi = x < y ? x : y, qi = x < y ? y : x;
                    if (qi < na) {
                        const double* lg = mylog + ((size_t)rr * H + tid) * 3;
                        const double c = lg[0];
                        const cd se = make_double2(lg[1], lg[2]);
                        const cd xp = pv[pi], xq = pv[qi];
                        const cd t1 = zmul(se, xq), t2 = zmul_conj(xp, se);          // s x_q, conj(s) x_p
                        pv[pi] = make_double2(c * xp.x + t1.x, c * xp.y + t1.y);
                        pv[qi] = make_double2(c * xq.x - t2.x, c * xq.y - t2.y);
                    }
                }
                __syncthreads();
            }
        }
        const double tr = sh_tr;
        const double lmax = fmax(red[1][0], 0.0);
        const double rho = sqrt(lmax);                       // (unclamped above: q = M^H p / rho has unit norm)
        const bool defined = !bad && tr > 0.0 && rho > 0.0;                   // (B = 0 exactly: coherences 0, no vectors)
        // q = M^H p / rho_1, the filters' right-hand sides, then the patterns L p, L q in place of p, q
        for (int j = tid; j < nb; j += 256) {
            cd sacc = make_double2(0.0, 0.0);
            for (int i = 0; i < na; ++i) { const cd t = zmul_conj(pv[i], PM[i * ld + j]); sacc.x += t.x; sacc.y += t.y; }
            const cd qj = make_double2(sacc.x / rho, sacc.y / rho);
            qv[j] = qj; xb[j] = qj;
        }
        for (int i = tid; i < na; i += 256) xa[i] = pv[i];
        __syncthreads();
        cd pat = make_double2(0.0, 0.0);
        if (tid < 128) { if (tid < na) for (int k = 0; k <= tid; ++k) { const cd t = zmul(PA[tid * ld + k], pv[k]); pat.x += t.x; pat.y += t.y; } }
        else { const int j = tid - 128; if (j < nb) for (int k = 0; k <= j; ++k) { const cd t = zmul(PB[j * ld + k], qv[k]); pat.x += t.x; pat.y += t.y; } }
        __syncthreads();
        if (tid < 128) { if (tid < na) pv[tid] = pat; }
        else if (tid - 128 < nb) qv[tid - 128] = pat;
        cv_back_substitute(PA, PB, ld, ld, na, nb, xa, xb, tid);
        if (tid == 0) {
            const cd* lowp = flip ? qv : pv;                 // the pattern of the group with the lower label
            const int nl = flip ? nb : na;
            double best = -1.0;
            cd val = make_double2(1.0, 0.0);
            for (int i = 0; i < nl; ++i) { const double m2 = lowp[i].x * lowp[i].x + lowp[i].y * lowp[i].y; if (m2 > best) { best = m2; val = lowp[i]; } }
            const double ab = sqrt(best);
            sh_phase = ab > 0.0 ? make_double2(val.x / ab, -val.y / ab) : make_double2(1.0, 0.0);
            double* o = a.out + bin * a.G * a.G;
            const double m = bad ? nan("") : fmin(rho, 1.0);
            o[ga * a.G + gb] = m;
            o[gb * a.G + ga] = m;
            if (bad) atomicAdd(a.fail, 1);
        }
        __syncthreads();
        const size_t oa = (((size_t)bin * a.G + ga) * a.G + gb) * v.vstride, ob = (((size_t)bin * a.G + gb) * a.G + ga) * v.vstride;
        if (!bad) {                                          // (the outputs are NaN-filled before the launch)
            for (int k = tid; k < na; k += 256) {
                const double r = sqrt(fmin(fmax(red[1][k], 0.0), 1.0));
                v.coherences[oa + k] = r; v.coherences[ob + k] = r;
            }
        }
        if (defined) {
            const cd ph = sh_phase;
            for (int i = tid; i < na; i += 256) { v.filters[oa + i] = zmul(xa[i], ph); v.patterns[oa + i] = zmul(pv[i], ph); }
            for (int j = tid; j < nb; j += 256) { v.filters[ob + j] = zmul(xb[j], ph); v.patterns[ob + j] = zmul(qv[j], ph); }
        }
        __syncthreads();
    }
}

extern "C" int sc_canonical_max_group(void) { return CBIG_C; }

// what both launch functions check and fill in
static int canonical_args(const char* what, const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                          int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes, int n_groups, int max_group_size,
                          double* d_out, double* d_out_mim, int32_t* d_fail, CanonArgs* out) {
    CanonArgs& a = *out;
    const int rcv = sc_csm_view(planes, n_bins, n_bins, n_signals, n_observations, &a.v);
    if (rcv != SC_OK) return rcv;
    SC_REQUIRE(n_groups >= 1 && n_bins >= 1, "empty problem");
    if (max_group_size > CBIG_C) {
        sc_set_error("%s supports groups of at most %d channels (got %d)", what, CBIG_C, max_group_size);
        return SC_EUNSUPPORTED;
    }
    a.accum = sc_rec(d_accum, planes); a.members = d_members; a.sizes = d_sizes; a.out = d_out; a.fail = d_fail;
    a.out_mim = d_out_mim;
    a.n_bins = n_bins; a.G = n_groups; a.n_gpairs = n_groups * (n_groups - 1) / 2;
    a.mstride = max_group_size <= 32 ? 32 : CBIG_C;      // (the member table's row length is the caller's: sc_hip.h)
    a.jtol = 1e-24;          // off^2 <= jtol dia^2: eigenvalues to ~1e-12 relative (quadratic convergence)
    return SC_OK;
}

// The launches of both entry points: the tier of the largest group (<= 16 channels: factor + pair kernels; <= 64: a workgroup per
// pair in LDS; <= 128: the same with the blocks in a global scratch) and its workspace.  IM: the interaction view, MIC into `out`
// and MIM into `out_mim`; it always takes the Householder / Sturm kernels (SC_CANON_EIG=jacobi selects the Jacobi kernels of
// canonical coherence only).  The entry points check their pointers first.
template <bool IM>
static int canonical_launch(const char* what, const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                            int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes, int n_groups,
                            int max_group_size, double* d_out, double* d_out_mim, int32_t* d_fail, void* stream) {
    CanonArgs a;
    const int rca = canonical_args(what, d_accum, n_bins, n_signals, planes, n_observations, d_members, d_sizes, n_groups,
                                   max_group_size, d_out, d_out_mim, d_fail, &a);
    if (rca != SC_OK) return rca;
    hipStream_t st = (hipStream_t)stream;
    const int64_t total_out = n_bins * n_groups * n_groups;
    sc_internal_fill_nan(d_out, total_out, st);
    if (IM) sc_internal_fill_nan(d_out_mim, total_out, st);
    (void)hipMemsetAsync(d_fail, 0, 4, st);
    const int64_t threads = n_bins * a.n_gpairs;
    // (SC_CANON_EIG=jacobi: the parallel Jacobi kernels of rounds 1-4, every eigenvalue of B -- canonical coherence only, A/B and
    //  cross-check)
    const char* eig = sc_switch(SC_SW_CANON_EIG);
    const bool jacobi = !IM && eig && eig[0] == 'j';
    if (threads > 0) {
        const unsigned blocks = (unsigned)((threads + 63) / 64);
        // members stride must match the instantiated CMAX
        if (max_group_size <= 16) {
            // group factors once per bin into a stream-ordered workspace, then a wave per (bin, group pair)
            cd* Lg = nullptr;
            const size_t lg_bytes = (size_t)n_bins * n_groups * CB_C * CB_C * sizeof(cd);
            const size_t ok_bytes = (((size_t)n_bins * n_groups * sizeof(int)) + 255) & ~(size_t)255;
            if (hipMallocAsync((void**)&Lg, lg_bytes + ok_bytes, st) != hipSuccess) {
                sc_set_error("%s: workspace allocation of %zu bytes failed", what, lg_bytes + ok_bytes);
                return SC_ENOMEM;
            }
            int* okb = reinterpret_cast<int*>(reinterpret_cast<char*>(Lg) + lg_bytes);
            const size_t lds_f = (size_t)CB_WAVES * CB_C * CB_C * sizeof(cd);
            const size_t lds_p = (size_t)CB_WAVES * 2 * CB_C * CB_C * sizeof(cd) + CB_WAVES * 24 * 8;
            (void)hipFuncSetAttribute((const void*)canonical_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p);
            hipLaunchKernelGGL(canonical_factor_kernel<IM>, dim3((unsigned)n_bins), dim3(64 * CB_WAVES), lds_f, st, a, Lg, okb);
            const int64_t n_gp = a.n_gpairs;
            const int64_t n_wg = ((n_gp + CB_WAVES - 1) / CB_WAVES) * n_bins;
            if (n_wg > 0x7fffffffLL) { (void)hipFreeAsync(Lg, st); sc_set_error("%s: too many (bin, pair) tasks", what); return SC_EINVAL; }
            if (jacobi) {
                hipLaunchKernelGGL(canonical_pair_kernel, dim3((unsigned)n_wg), dim3(64 * CB_WAVES), lds_p, st, a, (const cd*)Lg,
                                   (const int*)okb);
            } else {
                const size_t lds_h = (size_t)CB_WAVES * (2 * CB_C * CB_C + 32) * sizeof(cd);
                (void)hipFuncSetAttribute((const void*)canonical_pair_hh_kernel<IM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_h);
                hipLaunchKernelGGL(canonical_pair_hh_kernel<IM>, dim3((unsigned)n_wg), dim3(64 * CB_WAVES), lds_h, st, a, (const cd*)Lg,
                                   (const int*)okb);
            }
            (void)hipFreeAsync(Lg, st);
        } else if (max_group_size <= 32 && jacobi) {
            // (rounds 1-5: a wave per problem, its three blocks in the lanes' scratch, Jacobi -- 134 ms for 8 groups of 32 x 513 bins
            //  where the workgroup-per-problem kernel below takes 22: kept for A/B and cross-check only)
            hipLaunchKernelGGL(canonical_kernel<32>, dim3(blocks), dim3(64), 0, st, a);
        } else if (max_group_size <= CBH_SMALL && !jacobi) {
            // every pair fits LDS: no scratch, and as many persistent workgroups per compute unit as their LDS allows
            const int sn = max_group_size, sld = max_group_size | 1;
            const size_t lds = (size_t)2 * sn * sld * sizeof(cd);
            int per_cu = (int)((160 * 1024 - 8 * 1024) / (lds + 7 * 1024));          // (static arrays: ~7 KB a workgroup)
            per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
            const int64_t want = (int64_t)256 * per_cu;
            const int slots = (int)(threads < want ? threads : want);
            SC_CHECK_HIP(hipFuncSetAttribute((const void*)canonical_big_hh_kernel<IM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(canonical_big_hh_kernel<IM>, dim3((unsigned)slots), dim3(256), lds, st, a, (cd*)nullptr, threads, sn, sld);
        } else {
            // (members stride CBIG_C) persistent workgroups, three C x C matrices each in a stream-ordered scratch
            const int slots = (int)(threads < 256 ? threads : 256);
            cd* scratch = nullptr;
            const size_t sbytes = (size_t)slots * 3 * CBIG_C * CBIG_C * sizeof(cd);
            if (hipMallocAsync((void**)&scratch, sbytes, st) != hipSuccess) {
                sc_set_error("%s: scratch allocation of %zu bytes failed", what, sbytes);
                return SC_ENOMEM;
            }
            if (jacobi) {                  // (the round-2 kernel, every eigenvalue of B -- A/B and cross-check)
                constexpr size_t HM = CBIG_C / 2;
                const size_t lds = (size_t)CBIG_C * (CBIG_C + 1) / 2 * sizeof(cd) + HM * 8 + HM * 16 + 2 * HM * 4 +
                                   HM * (HM + 1) * 2 + 64;
                SC_CHECK_HIP(hipFuncSetAttribute((const void*)canonical_big_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(canonical_big_kernel, dim3((unsigned)slots), dim3(256), lds, st, a, scratch, threads);
            } else {
                const size_t lds = (size_t)CBH_LDS_N * CBH_LDS_N * sizeof(cd);
                SC_CHECK_HIP(hipFuncSetAttribute((const void*)canonical_big_hh_kernel<IM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(canonical_big_hh_kernel<IM>, dim3((unsigned)slots), dim3(256), lds, st, a, scratch, threads, CBH_SMALL, CBH_LD);
            }
            (void)hipFreeAsync(scratch, st);
        }
    }
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}

extern "C" int sc_canonical_coherence_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                          int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                          int n_groups, int max_group_size, double* d_out, int32_t* d_fail,
                                          void* stream) {
    ScTimed timed_("canonical_coherence", stream);
    SC_REQUIRE(d_accum && d_members && d_sizes && d_out && d_fail, "NULL argument");
    return canonical_launch<false>("canonical coherence", d_accum, n_bins, n_signals, planes, n_observations, d_members, d_sizes,
                                   n_groups, max_group_size, d_out, nullptr, d_fail, stream);
}

extern "C" int sc_imaginary_interaction_vectors_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                                    int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                                    int n_groups, int max_group_size, double* d_mic, double* d_filters,
                                                    double* d_patterns, int32_t* d_fail, void* stream) {
    ScTimed timed_("imaginary_interaction_vectors", stream);
    const char* what = "imaginary interaction vectors";
    SC_REQUIRE(d_accum && d_members && d_sizes && d_mic && d_filters && d_patterns && d_fail, "NULL argument");
    SC_REQUIRE(max_group_size >= 1, "empty groups");
    CanonArgs a;
    const int rca = canonical_args(what, d_accum, n_bins, n_signals, planes, n_observations, d_members, d_sizes, n_groups,
                                   max_group_size, d_mic, nullptr, d_fail, &a);
    if (rca != SC_OK) return rca;
    if (max_group_size <= CB_C) a.mstride = CB_C;
    hipStream_t st = (hipStream_t)stream;
    const int64_t total_out = n_bins * n_groups * n_groups;
    sc_internal_fill_nan(d_mic, total_out, st);
    sc_internal_fill_nan(d_filters, total_out * max_group_size, st);
    sc_internal_fill_nan(d_patterns, total_out * max_group_size, st);
    (void)hipMemsetAsync(d_fail, 0, 4, st);
    const int64_t items = n_bins * a.n_gpairs;
    if (items > 0) {
        IvArgs v;
        v.filters = d_filters; v.patterns = d_patterns; v.vstride = max_group_size; v.bn = max_group_size;
        v.lds_n = iv_lds_n(max_group_size); v.lds_ld = v.lds_n | 1;
        const size_t lds = iv_lds_bytes(v.bn, v.lds_n);
        int per_cu = (int)(IV_LDS_LIMIT / (lds + IV_STATIC_LDS));      // persistent workgroups a compute unit holds by LDS
        per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
        const int64_t want = (int64_t)256 * per_cu;
        const int slots = (int)(items < want ? items : want);
        const int Mb = v.bn + (v.bn & 1);
        const size_t log_bytes = ((size_t)IV_SWEEPS * (Mb - 1) * (Mb / 2) * 3 * sizeof(double) * slots + 255) & ~(size_t)255;
        const size_t sbytes = v.lds_n < max_group_size ? (size_t)slots * 3 * CBIG_C * CBIG_C * sizeof(cd) : 0;
        char* work = nullptr;
        if (hipMallocAsync((void**)&work, log_bytes + sbytes, st) != hipSuccess) {
            sc_set_error("%s: workspace allocation of %zu bytes failed", what, log_bytes + sbytes);
            return SC_ENOMEM;
        }
        v.log = reinterpret_cast<double*>(work);
        v.scratch = sbytes ? reinterpret_cast<cd*>(work + log_bytes) : nullptr;
        const hipError_t rcl = hipFuncSetAttribute((const void*)interaction_vectors_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rcl == hipSuccess) hipLaunchKernelGGL(interaction_vectors_kernel, dim3((unsigned)slots), dim3(256), lds, st, a, v, items);
        (void)hipFreeAsync(work, st);
        SC_CHECK_HIP(rcl);
    }
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}

extern "C" int sc_canonical_coherence_vectors_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                                  int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                                  int n_groups, int max_group_size, double* d_coherence, double* d_coherences,
                                                  double* d_filters, double* d_patterns, int32_t* d_fail, void* stream) {
    ScTimed timed_("canonical_coherence_vectors", stream);
    const char* what = "canonical coherence vectors";
    SC_REQUIRE(d_accum && d_members && d_sizes && d_coherence && d_coherences && d_filters && d_patterns && d_fail, "NULL argument");
    SC_REQUIRE(max_group_size >= 1, "empty groups");
    CanonArgs a;
    const int rca = canonical_args(what, d_accum, n_bins, n_signals, planes, n_observations, d_members, d_sizes, n_groups,
                                   max_group_size, d_coherence, nullptr, d_fail, &a);
    if (rca != SC_OK) return rca;
    if (max_group_size <= CB_C) a.mstride = CB_C;
    hipStream_t st = (hipStream_t)stream;
    const int64_t total_out = n_bins * n_groups * n_groups;
    sc_internal_fill_nan(d_coherence, total_out, st);
    sc_internal_fill_nan(d_coherences, total_out * max_group_size, st);
    sc_internal_fill_nan(d_filters, total_out * max_group_size * 2, st);
    sc_internal_fill_nan(d_patterns, total_out * max_group_size * 2, st);
    (void)hipMemsetAsync(d_fail, 0, 4, st);
    const int64_t items = n_bins * a.n_gpairs;
    if (items > 0) {
        CvArgs v;
        v.coherences = d_coherences;
        v.filters = reinterpret_cast<cd*>(d_filters); v.patterns = reinterpret_cast<cd*>(d_patterns);
        v.vstride = max_group_size; v.bn = max_group_size;
        v.lds_n = iv_lds_n(max_group_size, sizeof(cd)); v.lds_ld = v.lds_n | 1;
        const size_t lds = iv_lds_bytes(v.bn, v.lds_n, sizeof(cd));
        int per_cu = (int)(IV_LDS_LIMIT / (lds + IV_STATIC_LDS));      // persistent workgroups a compute unit holds by LDS,
        per_cu = per_cu < 1 ? 1 : (per_cu > 3 ? 3 : per_cu);           // and by registers (130 VGPRs: 3 waves a SIMD)
        const int64_t want = (int64_t)256 * per_cu;
        const int slots = (int)(items < want ? items : want);
        const int Mb = v.bn + (v.bn & 1);
        const size_t log_bytes = ((size_t)IV_SWEEPS * (Mb - 1) * (Mb / 2) * 3 * sizeof(double) * slots + 255) & ~(size_t)255;
        const size_t sbytes = v.lds_n < max_group_size ? (size_t)slots * 3 * CBIG_C * CBIG_C * sizeof(cd) : 0;
        char* work = nullptr;
        if (hipMallocAsync((void**)&work, log_bytes + sbytes, st) != hipSuccess) {
            sc_set_error("%s: workspace allocation of %zu bytes failed", what, log_bytes + sbytes);
            return SC_ENOMEM;
        }
        v.log = reinterpret_cast<double*>(work);
        v.scratch = sbytes ? reinterpret_cast<cd*>(work + log_bytes) : nullptr;
        const hipError_t rcl = hipFuncSetAttribute((const void*)canonical_vectors_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rcl == hipSuccess) hipLaunchKernelGGL(canonical_vectors_kernel, dim3((unsigned)slots), dim3(256), lds, st, a, v, items);
        (void)hipFreeAsync(work, st);
        SC_CHECK_HIP(rcl);
    }
    SC_CHECK_HIP(hipGetLastError());
    return SC_OK;
}

extern "C" int sc_imaginary_interaction_f64(const void* d_accum, int64_t n_bins, int64_t n_signals, uint32_t planes,
                                            int64_t n_observations, const int32_t* d_members, const int32_t* d_sizes,
                                            int n_groups, int max_group_size, double* d_mic, double* d_mim,
                                            int32_t* d_fail, void* stream) {
    ScTimed timed_("imaginary_interaction", stream);
    SC_REQUIRE(d_accum && d_members && d_sizes && d_mic && d_mim && d_fail, "NULL argument");
    return canonical_launch<true>("imaginary interaction", d_accum, n_bins, n_signals, planes, n_observations, d_members, d_sizes,
                                  n_groups, max_group_size, d_mic, d_mim, d_fail, stream);
}
