// sc_jackknife.hip -- delete-one jackknife of power, Fisher-z coherence, imaginary coherence and the phase-lag family (gfx950).
//
// For a kept index and bin, delete units u = 1 .. n of g observations each: G_u = sum over the unit's observations of
// x_i conj(x_j), S = sum_u G_u (the un-normalised CSM record the package accumulates anyway), S_(-u) = S - G_u.  Leaving a
// unit out therefore needs no second pass over the data: one read of the spectra, and per (unit, channel pair, bin) one small
// epilogue d_u = theta(S - G_u) - theta(S).  The kernel returns theta(S), sum_u d_u and sum_u d_u^2; the host finishes
// (m = sum d / n, sum (d - m)^2 = sum d^2 - n m^2: d is already centred on the full estimate, so m is of the order of d).
//
// The walk (jk_place, jk_walk), the same for every kernel here: one workgroup of 256 threads owns (bin, pair of 32-channel tiles,
// share of the units); a thread owns 2 x 2 entries (i, j) of the tile pair.  The rows of the two channel tiles are staged in LDS 32
// observations at a time, and the walk hands every observation to the kernel's per-row callable as (x_i[2], x_j[2]) and calls its
// per-unit callable after the g-th row of a unit.  The tile pairs of a bin are consecutive workgroups, so a bin's rows come from
// HBM once and from cache for the other pairs.  Where bins x tile pairs do not fill the chip the units are split over gridDim.y
// workgroups that write partial sums to the workspace, added in split order by a second kernel: no floating-point atomics
// anywhere, results are bit-identical from run to run.  A kernel is what it keeps in registers and its two callables:
//
// jk_kernel: the totals S_ii, S_jj, S_ij of the record.  Per row: G_u and the two powers, summed in the engine's precision (f32
// products for complex64 spectra, f64 for complex128).  Per unit: the subtraction, d_u of every measure and its two sums, in
// fp64 on both engines.  Only i < j is evaluated; the mirror entry is written with it (imaginary coherence: negated).
//
// jk_phase_kernel, the phase-lag family.  Per row: JkPhaseUnit::add -- Im s = Im(x_i conj(x_j)) is formed once and summed per unit
// as a_u = sum Im s, b_u = sum |Im s|, c_u = sum sign(Im s) (an integer) and q_u = sum (Im s)^2.  Per unit: the totals A, B, N, Q
// are the planes SC_PLANE_CSM (im), _ABS_IM, _SIGN_IM and _IM_SQ of the accumulator record, and with n = n_units_total g observations
//     PLI = N / n,  wPLI = (A / n) / w with w = B / n (1 where w < 2^-52),  debiased PLI^2 = (n PLI^2 - 1) / (n - 1),
//     debiased wPLI^2 = (A^2 - Q) / (B^2 - Q) (NaN where the denominator is exactly 0)
// on the identity scale; a delete-one value is the same formula on A - a_u, ... and n' = (n_units_total - 1) g.
//
// jk_phase_totals_kernel sums such a record from the spectra.  Per row: the same JkPhaseUnit::add; per unit: the unit sums added
// in fp64.  Both kernels run the one walk and the one JkPhaseUnit, so a total is by construction the fp64 sum of the very unit
// sums that are subtracted from it.  It is what the hosts hand in, because the float32 engine's own records are too coarse in A
// for the debiased wPLI^2 of a pair near 0.
#include "sc_jackknife_value.h"

namespace {

constexpr int JK_T = 32;        // channel tile edge of a workgroup (2 x 2 entries per thread)
constexpr int JK_ROWS = 32;     // observation rows staged per barrier pair
constexpr int JK_MAX_SPLITS = 256;
constexpr int JK_MAX_BLOCKS = 4;  // measure blocks of one call (three of jk_kernel, four of jk_phase_kernel)
constexpr uint32_t JK_PHASE_ALL = SC_JACKKNIFE_PHASE_PLI | SC_JACKKNIFE_PHASE_WPLI | SC_JACKKNIFE_PHASE_DEBIASED_PLI2 |
                                  SC_JACKKNIFE_PHASE_DEBIASED_WPLI2;

// what the walk and the write-out of every kernel need (jk_geometry fills it)
struct JkGeom {
    ScAxes a;
    int NB16, n_tiles16;
    int64_t rec_stride;          // elements of one bin record
    int n_freq, NT, n_tp;
    int over, g, q_tapers;       // rows per unit; tapers per window inside a unit (over = trials)
    int64_t unit_begin, unit_end, units_per_split;
    int64_t n_bins;
    int64_t out_doubles;
    double* out;                 // split s writes at out + s * out_doubles
};

// a thread's place: the entries (ci[a], cj[b]), a, b = 0, 1, of the tile pair (ti, tj) of bin `bin`, whose rows start x_off
// elements into the spectra
struct JkPlace {
    int tx, ty, ti, tj, ci[2], cj[2];
    int64_t bin, x_off;
};

__device__ __forceinline__ JkPlace jk_place(const JkGeom& p) {
    JkPlace w;
    w.tx = threadIdx.x & 15;
    w.ty = threadIdx.x >> 4;
    const int64_t wg = blockIdx.x;
    const int tp = (int)(wg % p.n_tp);
    w.bin = wg / p.n_tp;
    int ti = 0, rem = tp;
    while (rem >= p.NT - ti) { rem -= p.NT - ti; ++ti; }
    w.ti = ti;
    w.tj = ti + rem;
    const int f = (int)(w.bin % p.n_freq), grp = (int)(w.bin / p.n_freq);
    w.x_off = (int64_t)f * p.a.sF + sc_group_offset(p.a, grp);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        w.ci[a] = w.ti * JK_T + w.ty + 16 * a;
        w.cj[a] = w.tj * JK_T + w.tx + 16 * a;
    }
    return w;
}

__device__ __forceinline__ int64_t jk_row_offset(const JkGeom& p, int64_t u, int q) {
    return jk_unit_row_offset(p.a, p.over, p.q_tapers, u, q);
}

// The units of this workgroup's split, row by row: row(xi, xj) for every observation (the two entries of either channel tile
// this thread owns; channels past C read as 0), unit() after the last row of every unit.
template <typename T2, typename Row, typename Unit>
__device__ __forceinline__ void jk_walk(const T2* __restrict__ X, const JkGeom& p, const JkPlace& w, Row row, Unit unit) {
    __shared__ T2 rows[JK_ROWS][2 * JK_T];
    __shared__ int64_t row_off[JK_ROWS];      // element offset of every staged row: one decode per row, not per element
    const int tid = threadIdx.x, tx = w.tx, ty = w.ty, ti = w.ti, tj = w.tj;
    const T2* Xb = X + w.x_off;
    const int C = p.a.C;
    const int64_t u0 = p.unit_begin + (int64_t)blockIdx.y * p.units_per_split;
    const int64_t u1 = u0 + p.units_per_split < p.unit_end ? u0 + p.units_per_split : p.unit_end;
    const int n_rows = (int)((u1 - u0) * p.g);
    int cnt = 0;
    for (int r0 = 0; r0 < n_rows; r0 += JK_ROWS) {
        const int nr = n_rows - r0 < JK_ROWS ? n_rows - r0 : JK_ROWS;
        __syncthreads();
        if (tid < nr) {
            const int q = r0 + tid, du = q / p.g;
            row_off[tid] = jk_row_offset(p, u0 + du, q - du * p.g);
        }
        __syncthreads();
        for (int e = tid; e < nr * 2 * JK_T; e += 256) {
            const int r = e >> 6, col = e & 63;
            const int c = (col < JK_T ? ti : tj) * JK_T + (col & (JK_T - 1));
            T2 v;
            v.x = 0; v.y = 0;
            if (c < C) v = Xb[row_off[r] + c];
            rows[r][col] = v;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            T2 xi[2], xj[2];
            xi[0] = rows[r][ty]; xi[1] = rows[r][ty + 16];
            xj[0] = rows[r][JK_T + tx]; xj[1] = rows[r][JK_T + tx + 16];
            row(xi, xj);
            if (++cnt == p.g) {
                cnt = 0;
                unit();
            }
        }
    }
}

// element (i, j), i <= j, of a plane of a bin record: upper-triangular 16 x 16 tiles
__device__ __forceinline__ int64_t jk_tile_offset(int i, int j, int NB16) {
    return (int64_t)sc_tile_index(i >> 4, j >> 4, NB16) * SC_TILE_ELEMS + (i & 15) * 16 + (j & 15);
}

struct JkArgs {
    JkGeom geo;
    ScRec total;
    int p_csm;
    double n_total, ln_ratio;    // units of the whole job, ln(n / (n - 1))
    uint32_t measures;
    int64_t off[3];              // first double of each measure's block, -1: not requested
};

// S_ij (i <= j) of the total record: re and im planes
__device__ __forceinline__ void jk_total(const ScRec& rec, const JkArgs& p, int i, int j, double& re, double& im) {
    const int64_t off = jk_tile_offset(i, j, p.geo.NB16);
    const int64_t plane = (int64_t)p.geo.n_tiles16 * SC_TILE_ELEMS;
    re = rec[p.p_csm * plane + off];
    im = rec[(p.p_csm + 1) * plane + off];
}

template <typename T, typename T2>
__global__ __launch_bounds__(256) void jk_kernel(const T2* __restrict__ X, JkArgs p) {
    const JkPlace w = jk_place(p.geo);
    const int (&ci)[2] = w.ci, (&cj)[2] = w.cj;
    const int64_t bin = w.bin;
    const int C = p.geo.a.C;
    const ScRec rec = p.total + bin * p.geo.rec_stride;
    const bool want_pow = p.measures & SC_JACKKNIFE_POWER, want_coh = p.measures & SC_JACKKNIFE_COHERENCE_MAGNITUDE,
               want_im = p.measures & SC_JACKKNIFE_IMAGINARY_COHERENCE;
    const bool diag_thread = w.ti == w.tj && w.tx == w.ty;
    const double nan = __builtin_nan(""), ln_ratio = p.ln_ratio;

    double Sii[2], Sjj[2], Sre[2][2], Sim[2][2], bcoh[2][2], bim[2][2];
    bool valid[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        double dummy;
        Sii[a] = Sjj[a] = 1.0;
        if (ci[a] < C) jk_total(rec, p, ci[a], ci[a], Sii[a], dummy);
        if (cj[a] < C) jk_total(rec, p, cj[a], cj[a], Sjj[a], dummy);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            valid[a][b] = ci[a] < cj[b] && cj[b] < C;
            Sre[a][b] = Sim[a][b] = 0.0;
            if (valid[a][b]) jk_total(rec, p, ci[a], cj[b], Sre[a][b], Sim[a][b]);
            const double rr = (1.0 / sqrt(Sii[a])) * (1.0 / sqrt(Sjj[b]));
            bcoh[a][b] = sqrt(Sre[a][b] * Sre[a][b] + Sim[a][b] * Sim[a][b]) * rr;
            bim[a][b] = Sim[a][b] * rr;
        }

    double coh1[2][2] = {}, coh2[2][2] = {}, im1[2][2] = {}, im2[2][2] = {}, pw1[2] = {}, pw2[2] = {};
    T Gre[2][2] = {}, Gim[2][2] = {}, Pi[2] = {}, Pj[2] = {};

    jk_walk(
        X, p.geo, w,
        [&](const T2 (&xi)[2], const T2 (&xj)[2]) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                Pi[a] += xi[a].x * xi[a].x + xi[a].y * xi[a].y;
                Pj[a] += xj[a].x * xj[a].x + xj[a].y * xj[a].y;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    Gre[a][b] += xi[a].x * xj[b].x + xi[a].y * xj[b].y;
                    Gim[a][b] += xi[a].y * xj[b].x - xi[a].x * xj[b].y;
                }
            }
        },
        [&, want_pow, want_coh, want_im, diag_thread, ln_ratio]() {   // (the flags by value: the loop then compiles as written in place)
            // the unit is complete: d_u = theta(S - G_u) - theta(S) of every measure, in fp64
            double ri[2], rj[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                ri[a] = 1.0 / sqrt(Sii[a] - (double)Pi[a]);
                rj[a] = 1.0 / sqrt(Sjj[a] - (double)Pj[a]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (valid[a][b]) {
                        const double re = Sre[a][b] - (double)Gre[a][b], im = Sim[a][b] - (double)Gim[a][b];
                        const double rr = ri[a] * rj[b];
                        if (want_coh) {
                            const double mag = sqrt(re * re + im * im) * rr;
                            const double d = jk_fisher_deviation(mag, bcoh[a][b]);
                            coh1[a][b] += d;
                            coh2[a][b] += d * d;
                        }
                        if (want_im) {
                            const double d = jk_imaginary_deviation(im, rr, bim[a][b]);
                            im1[a][b] += d;
                            im2[a][b] += d * d;
                        }
                    }
                    Gre[a][b] = 0; Gim[a][b] = 0;
                }
            if (want_pow && diag_thread) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    // ln((S - G) / ((n - 1) g)) - ln(S / (n g)) = log1p(-G / S) + ln(n / (n - 1))
                    const double d = log1p(-(double)Pi[a] / Sii[a]) + ln_ratio;
                    pw1[a] += d;
                    pw2[a] += d * d;
                }
            }
#pragma unroll
            for (int a = 0; a < 2; ++a) { Pi[a] = 0; Pj[a] = 0; }
        });

    double* out = p.geo.out + (int64_t)blockIdx.y * p.geo.out_doubles;
    const int64_t CC = (int64_t)C * C, plane2 = p.geo.n_bins * CC;
    if (want_coh) {
        double* th = out + p.off[1] + bin * CC;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (valid[a][b]) {
                    const int64_t e = (int64_t)ci[a] * C + cj[b], m = (int64_t)cj[b] * C + ci[a];
                    const double t = atanh(bcoh[a][b]);
                    th[e] = t; th[m] = t;
                    th[plane2 + e] = coh1[a][b]; th[plane2 + m] = coh1[a][b];
                    th[2 * plane2 + e] = coh2[a][b]; th[2 * plane2 + m] = coh2[a][b];
                }
    }
    if (want_im) {
        double* th = out + p.off[2] + bin * CC;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (valid[a][b]) {
                    const int64_t e = (int64_t)ci[a] * C + cj[b], m = (int64_t)cj[b] * C + ci[a];
                    th[e] = bim[a][b]; th[m] = -bim[a][b];
                    th[plane2 + e] = im1[a][b]; th[plane2 + m] = -im1[a][b];
                    th[2 * plane2 + e] = im2[a][b]; th[2 * plane2 + m] = im2[a][b];
                }
    }
    if (diag_thread) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (ci[a] >= C) continue;
            const int64_t e = (int64_t)ci[a] * C + ci[a];
            if (want_coh) {
                double* th = out + p.off[1] + bin * CC;
                th[e] = nan; th[plane2 + e] = nan; th[2 * plane2 + e] = nan;
            }
            if (want_im) {
                double* th = out + p.off[2] + bin * CC;
                th[e] = nan; th[plane2 + e] = nan; th[2 * plane2 + e] = nan;
            }
            if (want_pow) {
                double* th = out + p.off[0] + bin * C;
                const int64_t plane1 = p.geo.n_bins * C;
                th[ci[a]] = Sii[a] > 0.0 ? log(Sii[a] / (p.n_total * (double)p.geo.g)) : nan;
                th[plane1 + ci[a]] = Sii[a] > 0.0 ? pw1[a] : nan;
                th[2 * plane1 + ci[a]] = Sii[a] > 0.0 ? pw2[a] : nan;
            }
        }
    }
}

// ---- the phase-lag family ------------------------------------------------------------------------------------------------------
struct JkPhaseArgs {
    JkGeom geo;
    ScRec total;
    int p_im, p_abs, p_sq, p_sign;   // plane index of sum Im s, sum |Im s|, sum (Im s)^2, sum sign(Im s) in a bin record; -1: absent
    double n_full, n_del;            // observations of the full estimate and of a delete-one estimate
    uint32_t measures;
    int64_t off[JK_MAX_BLOCKS];      // first double of each measure's block, -1: not requested
};

// the sums of one unit over a thread's 2 x 2 entries, in the engine's precision: what jk_phase_kernel subtracts from the totals
// and what jk_phase_totals_kernel adds up to them
template <typename T>
struct JkPhaseUnit {
    T a[2][2], b[2][2], q[2][2];     // sum Im s, sum |Im s|, sum (Im s)^2
    int c[2][2];                     // sum sign(Im s)

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) { a[i][j] = 0; b[i][j] = 0; q[i][j] = 0; c[i][j] = 0; }
    }
    template <typename T2>
    __device__ __forceinline__ void add(const T2 (&xi)[2], const T2 (&xj)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const T im = xi[i].y * xj[j].x - xi[i].x * xj[j].y;
                a[i][j] += im;
                b[i][j] += im < 0 ? -im : im;
                q[i][j] += im * im;
                c[i][j] += (im > 0) - (im < 0);
            }
    }
};

// (the four statistics from the sums, the shifted sums and their move back to the origin: sc_jackknife_value.h)
template <typename T, typename T2>
__global__ __launch_bounds__(256) void jk_phase_kernel(const T2* __restrict__ X, JkPhaseArgs p) {
    const JkPlace w = jk_place(p.geo);
    const int (&ci)[2] = w.ci, (&cj)[2] = w.cj;
    const int64_t bin = w.bin;
    const int C = p.geo.a.C;
    const ScRec rec = p.total + bin * p.geo.rec_stride;
    const bool want_pli = p.measures & SC_JACKKNIFE_PHASE_PLI, want_wpli = p.measures & SC_JACKKNIFE_PHASE_WPLI,
               want_dpli = p.measures & SC_JACKKNIFE_PHASE_DEBIASED_PLI2, want_dwpli = p.measures & SC_JACKKNIFE_PHASE_DEBIASED_WPLI2;
    const bool diag_thread = w.ti == w.tj && w.tx == w.ty;
    const double nan = __builtin_nan("");
    const int64_t plane = (int64_t)p.geo.n_tiles16 * SC_TILE_ELEMS;

    bool valid[2][2];
    double tA[2][2], tB[2][2], tN[2][2], tQ[2][2];          // totals of the record
    double th[4][2][2];                                     // the full estimates
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            valid[a][b] = ci[a] < cj[b] && cj[b] < C;
            tA[a][b] = tB[a][b] = tN[a][b] = tQ[a][b] = 0.0;
            if (valid[a][b]) {
                const int64_t off = jk_tile_offset(ci[a], cj[b], p.geo.NB16);
                if (p.p_im >= 0) tA[a][b] = rec[p.p_im * plane + off];
                if (p.p_abs >= 0) tB[a][b] = rec[p.p_abs * plane + off];
                if (p.p_sq >= 0) tQ[a][b] = rec[p.p_sq * plane + off];
                if (p.p_sign >= 0) tN[a][b] = rec[p.p_sign * plane + off];
            }
            const double pli = jk_pli(tN[a][b], p.n_full);
            th[0][a][b] = pli;
            th[1][a][b] = jk_wpli(tA[a][b], tB[a][b], p.n_full);
            th[2][a][b] = jk_debiased_pli2(pli, p.n_full);
            th[3][a][b] = jk_debiased_wpli2(tA[a][b], tB[a][b], tQ[a][b]);
        }

    // The two sums are taken about the deviation of the first unit this workgroup walks, r (the shifted-data form), and moved back
    // to the origin after the last unit: sum d = k r + sum (d - r), sum d^2 = r sum d + sum (d - r)^2 + r sum (d - r).  A pair
    // whose units all have the same deviation (equal sign counts in every unit of a few) then gets sum d^2 = r sum d bit for
    // bit, which is what the host's n m^2 is: a standard error of exactly 0, as in exact arithmetic.
    double s1[4][2][2] = {}, s2[4][2][2] = {}, piv[4][2][2] = {};
    int n_done = 0;
    JkPhaseUnit<T> u;
    u.clear();

    jk_walk(
        X, p.geo, w, [&](const T2 (&xi)[2], const T2 (&xj)[2]) { u.add(xi, xj); },
        [&]() {
            // the unit is complete: d_u = theta(sums without the unit, n') - theta(sums, n) of every requested measure, in fp64
            const bool first = n_done == 0;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (!valid[a][b]) continue;
                    if (want_pli || want_dpli) {
                        const double pli = jk_pli(tN[a][b] - (double)u.c[a][b], p.n_del);
                        if (want_pli) jk_shifted_add(pli - th[0][a][b], first, piv[0][a][b], s1[0][a][b], s2[0][a][b]);
                        if (want_dpli)
                            jk_shifted_add(jk_debiased_pli2(pli, p.n_del) - th[2][a][b], first, piv[2][a][b], s1[2][a][b], s2[2][a][b]);
                    }
                    if (want_wpli || want_dwpli) {
                        const double A = tA[a][b] - (double)u.a[a][b], B = tB[a][b] - (double)u.b[a][b];
                        if (want_wpli) jk_shifted_add(jk_wpli(A, B, p.n_del) - th[1][a][b], first, piv[1][a][b], s1[1][a][b], s2[1][a][b]);
                        if (want_dwpli)
                            jk_shifted_add(jk_debiased_wpli2(A, B, tQ[a][b] - (double)u.q[a][b]) - th[3][a][b], first, piv[3][a][b],
                                           s1[3][a][b], s2[3][a][b]);
                    }
                }
            u.clear();
            ++n_done;
        });

#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                jk_shifted_finish(n_done, piv[m][a][b], s1[m][a][b], s2[m][a][b]);

    double* out = p.geo.out + (int64_t)blockIdx.y * p.geo.out_doubles;
    const int64_t CC = (int64_t)C * C, plane2 = p.geo.n_bins * CC;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (!(p.measures & (1u << m))) continue;
        double* o = out + p.off[m] + bin * CC;
        const double sgn = m < 2 ? -1.0 : 1.0;                // PLI and wPLI are antisymmetric, the debiased squares symmetric
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (valid[a][b]) {
                    const int64_t e = (int64_t)ci[a] * C + cj[b], mi = (int64_t)cj[b] * C + ci[a];
                    o[e] = th[m][a][b]; o[mi] = sgn * th[m][a][b];
                    o[plane2 + e] = s1[m][a][b]; o[plane2 + mi] = sgn * s1[m][a][b];
                    o[2 * plane2 + e] = s2[m][a][b]; o[2 * plane2 + mi] = s2[m][a][b];
                }
        if (diag_thread) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                if (ci[a] >= C) continue;
                const int64_t e = (int64_t)ci[a] * C + ci[a];
                o[e] = nan; o[plane2 + e] = nan; o[2 * plane2 + e] = nan;
            }
        }
    }
}

// The totals of the phase-lag family from the spectra themselves: the unit sums of jk_phase_kernel, added over the units in fp64
// and written as a record of doubles in the accumulator layout (upper 16 x 16 tiles; planes CSM (re = 0, im), ABS_IM, IM_SQ,
// SIGN_IM as requested).  So sum Im s = +-sum |Im s| bit for bit where every observation has the same sign, and there is no
// float32 summation error of thousands of observations in A, which the debiased wPLI^2 of a pair near 0 multiplies by B / A.
template <typename T, typename T2>
__global__ __launch_bounds__(256) void jk_phase_totals_kernel(const T2* __restrict__ X, JkPhaseArgs p) {
    const JkPlace w = jk_place(p.geo);
    double sA[2][2] = {}, sB[2][2] = {}, sQ[2][2] = {}, sN[2][2] = {};
    JkPhaseUnit<T> u;
    u.clear();

    jk_walk(
        X, p.geo, w, [&](const T2 (&xi)[2], const T2 (&xj)[2]) { u.add(xi, xj); },
        [&]() {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    sA[a][b] += (double)u.a[a][b]; sB[a][b] += (double)u.b[a][b];
                    sQ[a][b] += (double)u.q[a][b]; sN[a][b] += (double)u.c[a][b];
                }
            u.clear();
        });

    double* rec = p.geo.out + (int64_t)blockIdx.y * p.geo.out_doubles + w.bin * p.geo.rec_stride;
    const int64_t plane = (int64_t)p.geo.n_tiles16 * SC_TILE_ELEMS;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = w.ci[a], j = w.cj[b];
            if (!(i < j && j < p.geo.a.C)) continue;
            const int64_t off = jk_tile_offset(i, j, p.geo.NB16);
            if (p.p_im >= 0) rec[p.p_im * plane + off] = sA[a][b];
            if (p.p_abs >= 0) rec[p.p_abs * plane + off] = sB[a][b];
            if (p.p_sq >= 0) rec[p.p_sq * plane + off] = sQ[a][b];
            if (p.p_sign >= 0) rec[p.p_sign * plane + off] = sN[a][b];
        }
}

// partial sums of the unit splits -> the output, in split order; theta(S) is the same in every split.  A block is three arrays
// of `len` doubles from `off` on: theta(S), sum d, sum d^2.
struct JkFold {
    int n_blocks;
    int64_t off[JK_MAX_BLOCKS], len[JK_MAX_BLOCKS];
    int64_t out_doubles;
};

__global__ void jk_fold(const double* __restrict__ ws, int n_splits, JkFold f, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= f.out_doubles) return;
    bool is_theta = false;
#pragma unroll
    for (int m = 0; m < JK_MAX_BLOCKS; ++m)
        if (m < f.n_blocks && e >= f.off[m] && e < f.off[m] + f.len[m]) is_theta = true;
    double v = ws[e];
    if (!is_theta)
        for (int s = 1; s < n_splits; ++s) v += ws[(int64_t)s * f.out_doubles + e];
    out[e] = v;
}

struct JkPlan {
    ScAxes a;
    int64_t n_bins, n_units, g, out_doubles, off[JK_MAX_BLOCKS];
    int NT, n_tp, q_tapers, over;
};

// phase: the masks and blocks of the phase-lag family (four C x C blocks) instead of power / coherence / imaginary coherence
int jk_plan(const sc_spectra_desc* desc, uint32_t measures, int over, JkPlan* pl, bool phase = false) {
    SC_REQUIRE(desc, "NULL descriptor");
    if (sc_make_axes(desc, &pl->a) != SC_OK) return SC_EINVAL;
    const ScAxes& a = pl->a;
    SC_REQUIRE(a.F >= 1 && a.W >= 1 && a.R >= 1 && a.K >= 1 && a.C >= 1 && a.C <= 32768, "bad spectra sizes");
    if (phase)
        SC_REQUIRE(measures && !(measures & ~JK_PHASE_ALL),
                   "measures: a non-empty mask of SC_JACKKNIFE_PHASE_PLI, _WPLI, _DEBIASED_PLI2, _DEBIASED_WPLI2");
    else
        SC_REQUIRE(measures && !(measures & ~(SC_JACKKNIFE_POWER | SC_JACKKNIFE_COHERENCE_MAGNITUDE | SC_JACKKNIFE_IMAGINARY_COHERENCE)),
                   "measures: a non-empty mask of SC_JACKKNIFE_POWER, _COHERENCE_MAGNITUDE, _IMAGINARY_COHERENCE");
    SC_REQUIRE(over == SC_JACKKNIFE_OVER_TRIALS || over == SC_JACKKNIFE_OVER_OBSERVATIONS, "over: SC_JACKKNIFE_OVER_TRIALS or _OBSERVATIONS");
    pl->over = over;
    if (over == SC_JACKKNIFE_OVER_TRIALS) {
        SC_REQUIRE(desc->reduce_trial, "a jackknife over trials needs an expectation that averages over trials");
        pl->n_units = a.R;
        pl->g = (int64_t)a.rW * a.rK;
        pl->q_tapers = a.rK;
    } else {
        pl->n_units = a.n_obs;
        pl->g = 1;
        pl->q_tapers = 1;
    }
    pl->n_bins = (int64_t)a.n_groups * a.F;
    pl->NT = (a.C + JK_T - 1) / JK_T;
    pl->n_tp = pl->NT * (pl->NT + 1) / 2;
    SC_REQUIRE(pl->n_bins * pl->n_tp < (int64_t)1 << 31, "too many (bin, channel tile pair) workgroups for one launch");
    int64_t at = 0;
    for (int m = 0; m < JK_MAX_BLOCKS; ++m) {
        pl->off[m] = -1;
        if (measures & (1u << m)) {
            pl->off[m] = at;
            at += 3 * pl->n_bins * (m == 0 && !phase ? (int64_t)a.C : (int64_t)a.C * a.C);
        }
    }
    pl->out_doubles = at;
    return SC_OK;
}

// the blocks of a plan as jk_fold wants them
JkFold jk_fold_blocks(const JkPlan& pl, bool phase) {
    JkFold f = {};
    for (int m = 0; m < JK_MAX_BLOCKS; ++m)
        if (pl.off[m] >= 0) {
            f.off[f.n_blocks] = pl.off[m];
            f.len[f.n_blocks] = pl.n_bins * (m == 0 && !phase ? (int64_t)pl.a.C : (int64_t)pl.a.C * pl.a.C);
            ++f.n_blocks;
        }
    f.out_doubles = pl.out_doubles;
    return f;
}

// units per split and number of splits: only when bins x tile pairs leave compute units idle, and never fewer than 16 units each
void jk_splits(const JkPlan& pl, int64_t n_local, int64_t* per, int64_t* n_splits) {
    jk_unit_splits(pl.n_bins * pl.n_tp, n_local, JK_MAX_SPLITS, per, n_splits);
}

// bytes the splits of a unit range need for their partial sums (0: one split, no workspace; 0 too where the plan failed)
int64_t jk_workspace_bytes(int plan_rc, const JkPlan& pl, int64_t unit_begin, int64_t unit_end) {
    if (plan_rc != SC_OK || unit_end <= unit_begin) return 0;
    int64_t per, n_splits;
    jk_splits(pl, unit_end - unit_begin, &per, &n_splits);
    return n_splits > 1 ? n_splits * pl.out_doubles * (int64_t)sizeof(double) : 0;
}

// planes: of the record whose bins are rec_stride apart (the total a kernel reads, the record the totals kernel writes)
JkGeom jk_geometry(const JkPlan& pl, uint32_t planes, int64_t unit_begin, int64_t unit_end, int64_t per, double* out) {
    JkGeom p = {};
    p.a = pl.a;
    p.NB16 = sc_n_blocks(pl.a.C);
    p.n_tiles16 = sc_n_tiles(p.NB16);
    p.rec_stride = (int64_t)sc_plane_count(planes) * p.n_tiles16 * SC_TILE_ELEMS;
    p.n_freq = pl.a.F; p.NT = pl.NT; p.n_tp = pl.n_tp;
    p.over = pl.over; p.g = (int)pl.g; p.q_tapers = pl.q_tapers;
    p.unit_begin = unit_begin; p.unit_end = unit_end; p.units_per_split = per;
    p.n_bins = pl.n_bins;
    p.out_doubles = pl.out_doubles;
    p.out = out;
    return p;
}

// the unit range of a call against the plan's units
int jk_check_range(const JkPlan& pl, int64_t unit_begin, int64_t unit_end) {
    SC_REQUIRE(0 <= unit_begin && unit_begin < unit_end && unit_end <= pl.n_units, "unit range outside the spectra's units");
    return SC_OK;
}

// What the three entry points share once their own checks have passed and their own fields of *p are filled: the splits and their
// workspace, the geometry, the launch and the fold of the splits.  planes: see jk_geometry; zero: clear what the kernel writes into
// first (a record of totals).
template <typename T2, typename Args>
int jk_launch(void (*kernel)(const T2*, Args), const JkPlan& pl, Args* p, const void* d_X, uint32_t planes, int64_t unit_begin,
              int64_t unit_end, const JkFold& fold, bool zero, double* d_out, void* d_workspace, int64_t workspace_bytes,
              void* stream) {
    int64_t per, n_splits;
    jk_splits(pl, unit_end - unit_begin, &per, &n_splits);
    SC_REQUIRE(per * pl.g < (int64_t)1 << 31, "too many observation rows per workgroup");
    const int64_t out_bytes = pl.out_doubles * (int64_t)sizeof(double);
    if (n_splits > 1) SC_REQUIRE(d_workspace && workspace_bytes >= n_splits * out_bytes, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    p->geo = jk_geometry(pl, planes, unit_begin, unit_end, per, n_splits > 1 ? (double*)d_workspace : d_out);
    if (zero) SC_CHECK_HIP(hipMemsetAsync(p->geo.out, 0, (size_t)(n_splits * out_bytes), st));
    const dim3 grid((unsigned)(pl.n_bins * pl.n_tp), (unsigned)n_splits);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, (const T2*)d_X, *p);
    SC_CHECK_HIP(hipGetLastError());
    if (n_splits > 1) {
        hipLaunchKernelGGL(jk_fold, dim3((unsigned)((pl.out_doubles + 255) / 256)), dim3(256), 0, st, (const double*)d_workspace,
                           (int)n_splits, fold, d_out);
        SC_CHECK_HIP(hipGetLastError());
    }
    return SC_OK;
}

template <typename T, typename T2>
int jk_run(const void* d_X, const sc_spectra_desc* desc, const void* d_total, uint32_t planes, uint32_t measures, int over,
           int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out, void* d_workspace, int64_t workspace_bytes,
           void* stream) {
    ScTimed timed_("jackknife", stream);
    JkPlan pl;
    int rc = jk_plan(desc, measures, over, &pl);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(d_X && d_total && d_out, "NULL argument");
    SC_REQUIRE(planes & SC_PLANE_CSM, "the total record must contain SC_PLANE_CSM");
    if ((rc = jk_check_range(pl, unit_begin, unit_end)) != SC_OK) return rc;
    SC_REQUIRE(n_units_total >= 2 && n_units_total >= unit_end - unit_begin, "a jackknife needs at least two units");
    JkArgs p = {};
    p.total = sc_rec(d_total, planes);
    p.p_csm = sc_plane_offset(planes, SC_PLANE_CSM);
    p.n_total = (double)n_units_total;
    p.ln_ratio = log((double)n_units_total / (double)(n_units_total - 1));
    p.measures = measures;
    for (int m = 0; m < 3; ++m) p.off[m] = pl.off[m];
    return jk_launch(jk_kernel<T, T2>, pl, &p, d_X, planes, unit_begin, unit_end, jk_fold_blocks(pl, false), false, d_out,
                     d_workspace, workspace_bytes, stream);
}

// planes of the total record a mask of phase-lag measures reads
uint32_t jk_phase_planes(uint32_t measures) {
    uint32_t need = 0;
    if (measures & (SC_JACKKNIFE_PHASE_PLI | SC_JACKKNIFE_PHASE_DEBIASED_PLI2)) need |= SC_PLANE_SIGN_IM;
    if (measures & SC_JACKKNIFE_PHASE_WPLI) need |= SC_PLANE_CSM | SC_PLANE_ABS_IM;
    if (measures & SC_JACKKNIFE_PHASE_DEBIASED_WPLI2) need |= SC_PLANE_CSM | SC_PLANE_ABS_IM | SC_PLANE_IM_SQ;
    return need;
}

// the planes `use` of a record with the planes `planes`, where the phase-lag kernels find them
void jk_phase_plane_indices(JkPhaseArgs* p, uint32_t planes, uint32_t use) {
    p->p_im = (use & SC_PLANE_CSM) ? sc_plane_offset(planes, SC_PLANE_CSM) + 1 : -1;
    p->p_abs = (use & SC_PLANE_ABS_IM) ? sc_plane_offset(planes, SC_PLANE_ABS_IM) : -1;
    p->p_sq = (use & SC_PLANE_IM_SQ) ? sc_plane_offset(planes, SC_PLANE_IM_SQ) : -1;
    p->p_sign = (use & SC_PLANE_SIGN_IM) ? sc_plane_offset(planes, SC_PLANE_SIGN_IM) : -1;
}

template <typename T, typename T2>
int jk_phase_run(const void* d_X, const sc_spectra_desc* desc, const void* d_total, uint32_t planes, uint32_t measures, int over,
                 int64_t unit_begin, int64_t unit_end, int64_t n_units_total, double* d_out, void* d_workspace,
                 int64_t workspace_bytes, void* stream) {
    ScTimed timed_("jackknife_phase", stream);
    JkPlan pl;
    int rc = jk_plan(desc, measures, over, &pl, true);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(d_X && d_total && d_out, "NULL argument");
    const uint32_t need = jk_phase_planes(measures);
    SC_REQUIRE((planes & need) == need,
               "the total record lacks a plane of a requested measure (PLI, debiased PLI^2: SC_PLANE_SIGN_IM; wPLI: SC_PLANE_CSM | "
               "_ABS_IM; debiased wPLI^2: SC_PLANE_CSM | _ABS_IM | _IM_SQ)");
    if ((rc = jk_check_range(pl, unit_begin, unit_end)) != SC_OK) return rc;
    SC_REQUIRE(n_units_total >= 2 && n_units_total >= unit_end - unit_begin, "a jackknife needs at least two units");
    if (measures & (SC_JACKKNIFE_PHASE_DEBIASED_PLI2 | SC_JACKKNIFE_PHASE_DEBIASED_WPLI2))
        SC_REQUIRE((n_units_total - 1) * pl.g >= 2, "a debiased estimate needs at least two observations in a delete-one set");
    JkPhaseArgs p = {};
    p.total = sc_rec(d_total, planes);
    jk_phase_plane_indices(&p, planes, need);
    p.n_full = (double)n_units_total * (double)pl.g;
    p.n_del = (double)(n_units_total - 1) * (double)pl.g;
    p.measures = measures;
    for (int m = 0; m < JK_MAX_BLOCKS; ++m) p.off[m] = pl.off[m];
    return jk_launch(jk_phase_kernel<T, T2>, pl, &p, d_X, planes, unit_begin, unit_end, jk_fold_blocks(pl, true), false, d_out,
                     d_workspace, workspace_bytes, stream);
}

constexpr uint32_t JK_PHASE_PLANES_ALL = SC_PLANE_CSM | SC_PLANE_ABS_IM | SC_PLANE_IM_SQ | SC_PLANE_SIGN_IM;

// plan of a totals pass: the units and splits of jk_plan / jk_splits, no measure blocks
int jk_totals_plan(const sc_spectra_desc* desc, uint32_t planes, int over, JkPlan* pl) {
    const int rc = jk_plan(desc, SC_JACKKNIFE_PHASE_PLI, over, pl, true);
    if (rc != SC_OK) return rc;
    planes &= ~SC_RECORD_F64;
    SC_REQUIRE(planes && !(planes & ~JK_PHASE_PLANES_ALL), "planes: a non-empty set of SC_PLANE_CSM, _ABS_IM, _IM_SQ, _SIGN_IM");
    pl->out_doubles = pl->n_bins * (int64_t)sc_plane_count(planes) * sc_n_tiles(sc_n_blocks(pl->a.C)) * SC_TILE_ELEMS;
    return SC_OK;
}

template <typename T, typename T2>
int jk_phase_totals_run(const void* d_X, const sc_spectra_desc* desc, uint32_t planes, int over, int64_t unit_begin,
                        int64_t unit_end, double* d_record, void* d_workspace, int64_t workspace_bytes, void* stream) {
    ScTimed timed_("jackknife_phase_totals", stream);
    JkPlan pl;
    int rc = jk_totals_plan(desc, planes, over, &pl);
    if (rc != SC_OK) return rc;
    planes &= ~SC_RECORD_F64;
    SC_REQUIRE(d_X && d_record, "NULL argument");
    if ((rc = jk_check_range(pl, unit_begin, unit_end)) != SC_OK) return rc;
    JkPhaseArgs p = {};
    jk_phase_plane_indices(&p, planes, planes);
    JkFold fold = {};
    fold.out_doubles = pl.out_doubles;                  // (no theta blocks: every double is a sum over the splits)
    // zero: the entries no thread owns (the real plane, the diagonal and what lies below it in a diagonal tile, tile padding) are 0
    return jk_launch(jk_phase_totals_kernel<T, T2>, pl, &p, d_X, planes, unit_begin, unit_end, fold, true, d_record, d_workspace,
                     workspace_bytes, stream);
}

int jk_layout(int plan_rc, const JkPlan& pl, int64_t* n_bins, int64_t* n_units, int64_t* unit_size, int64_t* out_doubles) {
    if (plan_rc != SC_OK) return plan_rc;
    if (n_bins) *n_bins = pl.n_bins;
    if (n_units) *n_units = pl.n_units;
    if (unit_size) *unit_size = pl.g;
    if (out_doubles) *out_doubles = pl.out_doubles;
    return SC_OK;
}

}  // namespace

extern "C" int sc_jackknife_layout(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t* n_bins, int64_t* n_units,
                                   int64_t* unit_size, int64_t* out_doubles) {
    JkPlan pl;
    return jk_layout(jk_plan(desc, measures, over, &pl), pl, n_bins, n_units, unit_size, out_doubles);
}

extern "C" int64_t sc_jackknife_workspace_bytes(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t unit_begin,
                                                int64_t unit_end) {
    JkPlan pl;
    return jk_workspace_bytes(jk_plan(desc, measures, over, &pl), pl, unit_begin, unit_end);
}

extern "C" int sc_jackknife_f32(const void* d_X, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                                uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total,
                                double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return jk_run<float, float2>(d_X, desc, d_total, planes, measures, over, unit_begin, unit_end, n_units_total, d_out,
                                 d_workspace, workspace_bytes, stream);
}

extern "C" int sc_jackknife_f64(const void* d_X, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                                uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total,
                                double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return jk_run<double, double2>(d_X, desc, d_total, planes, measures, over, unit_begin, unit_end, n_units_total, d_out,
                                   d_workspace, workspace_bytes, stream);
}

extern "C" int sc_jackknife_phase_layout(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t* n_bins,
                                         int64_t* n_units, int64_t* unit_size, int64_t* out_doubles) {
    JkPlan pl;
    return jk_layout(jk_plan(desc, measures, over, &pl, true), pl, n_bins, n_units, unit_size, out_doubles);
}

extern "C" int64_t sc_jackknife_phase_workspace_bytes(const sc_spectra_desc* desc, uint32_t measures, int over,
                                                      int64_t unit_begin, int64_t unit_end) {
    JkPlan pl;
    return jk_workspace_bytes(jk_plan(desc, measures, over, &pl, true), pl, unit_begin, unit_end);
}

extern "C" int sc_jackknife_phase_f32(const void* d_X, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                                      uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total,
                                      double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return jk_phase_run<float, float2>(d_X, desc, d_total, planes, measures, over, unit_begin, unit_end, n_units_total, d_out,
                                       d_workspace, workspace_bytes, stream);
}

extern "C" int sc_jackknife_phase_f64(const void* d_X, const sc_spectra_desc* desc, const void* d_total, uint32_t planes,
                                      uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total,
                                      double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return jk_phase_run<double, double2>(d_X, desc, d_total, planes, measures, over, unit_begin, unit_end, n_units_total, d_out,
                                         d_workspace, workspace_bytes, stream);
}

extern "C" int64_t sc_jackknife_phase_totals_workspace_bytes(const sc_spectra_desc* desc, uint32_t planes, int over,
                                                             int64_t unit_begin, int64_t unit_end) {
    JkPlan pl;
    return jk_workspace_bytes(jk_totals_plan(desc, planes, over, &pl), pl, unit_begin, unit_end);
}

extern "C" int sc_jackknife_phase_totals_f32(const void* d_X, const sc_spectra_desc* desc, uint32_t planes, int over,
                                             int64_t unit_begin, int64_t unit_end, double* d_record, void* d_workspace,
                                             int64_t workspace_bytes, void* stream) {
    return jk_phase_totals_run<float, float2>(d_X, desc, planes, over, unit_begin, unit_end, d_record, d_workspace,
                                              workspace_bytes, stream);
}

extern "C" int sc_jackknife_phase_totals_f64(const void* d_X, const sc_spectra_desc* desc, uint32_t planes, int over,
                                             int64_t unit_begin, int64_t unit_end, double* d_record, void* d_workspace,
                                             int64_t workspace_bytes, void* stream) {
    return jk_phase_totals_run<double, double2>(d_X, desc, planes, over, unit_begin, unit_end, d_record, d_workspace,
                                                workspace_bytes, stream);
}
