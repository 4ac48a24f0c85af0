// sc_jackknife.hip -- delete-one jackknife of power, Fisher-z coherence and imaginary coherence (gfx950).
//
// For a kept index and bin, delete units u = 1 .. n of g observations each: G_u = sum over the unit's observations of
// x_i conj(x_j), S = sum_u G_u (the un-normalised CSM record the package accumulates anyway), S_(-u) = S - G_u.  Leaving a
// unit out therefore needs no second pass over the data: one read of the spectra, and per (unit, channel pair, bin) one small
// epilogue d_u = theta(S - G_u) - theta(S).  The kernel returns theta(S), sum_u d_u and sum_u d_u^2; the host finishes
// (m = sum d / n, sum (d - m)^2 = sum d^2 - n m^2: d is already centred on the full estimate, so m is of the order of d).
//
// One workgroup of 256 threads owns (bin, pair of 32-channel tiles, share of the units); a thread owns 2 x 2 entries (i, j) of
// the tile pair and keeps their totals, the running G_u and the two sums of every measure in registers.  The unit's rows of the
// two channel tiles are staged in LDS 32 rows at a time; G_u is summed in the engine's precision (f32 products for complex64
// spectra, f64 for complex128), the subtraction, the statistic and the sums are fp64 on both engines.  Only i < j is evaluated;
// the mirror entry is written with it (imaginary coherence: negated).  The tile pairs of a bin are consecutive workgroups, so a
// bin's rows come from HBM once and from cache for the other pairs.  Where bins x tile pairs do not fill the chip the units are
// split over gridDim.y workgroups that write partial sums to the workspace, added in split order by a second kernel: no
// floating-point atomics anywhere, results are bit-identical from run to run.
#include "sc_common.h"

#include <math.h>

namespace {

constexpr int JK_T = 32;        // channel tile edge of a workgroup (2 x 2 entries per thread)
constexpr int JK_ROWS = 32;     // observation rows staged per barrier pair
constexpr int JK_MAX_SPLITS = 256;

struct JkArgs {
    ScAxes a;
    ScRec total;
    int NB16, n_tiles16, p_csm;
    int64_t rec_stride;          // elements of one bin record
    int n_freq, NT, n_tp;
    int over, g, q_tapers;       // rows per unit; tapers per window inside a unit (over = trials)
    int64_t unit_begin, unit_end, units_per_split;
    double n_total, ln_ratio;    // units of the whole job, ln(n / (n - 1))
    uint32_t measures;
    int64_t n_bins;
    int64_t off[3];              // first double of each measure's block, -1: not requested
    int64_t out_doubles;
    double* out;                 // split s writes at out + s * out_doubles
};

__device__ __forceinline__ int64_t jk_row_offset(const JkArgs& p, int64_t u, int q) {
    if (p.over == SC_JACKKNIFE_OVER_OBSERVATIONS) return sc_obs_offset(p.a, (int)u);
    const int w = q / p.q_tapers, k = q - w * p.q_tapers;
    return (int64_t)w * p.a.sW + u * p.a.sR + (int64_t)k * p.a.sK;
}

// S_ij (i <= j) of the total record: upper-triangular 16 x 16 tiles, re and im planes
__device__ __forceinline__ void jk_total(const ScRec& rec, const JkArgs& p, int i, int j, double& re, double& im) {
    const int64_t off = (int64_t)sc_tile_index(i >> 4, j >> 4, p.NB16) * SC_TILE_ELEMS + (i & 15) * 16 + (j & 15);
    const int64_t plane = (int64_t)p.n_tiles16 * SC_TILE_ELEMS;
    re = rec[p.p_csm * plane + off];
    im = rec[(p.p_csm + 1) * plane + off];
}

template <typename T, typename T2>
__global__ __launch_bounds__(256) void jk_kernel(const T2* __restrict__ X, JkArgs p) {
    __shared__ T2 rows[JK_ROWS][2 * JK_T];
    __shared__ int64_t row_off[JK_ROWS];      // element offset of every staged row: one decode per row, not per element
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t wg = blockIdx.x;
    const int tp = (int)(wg % p.n_tp);
    const int64_t bin = wg / p.n_tp;
    int ti = 0, rem = tp;
    while (rem >= p.NT - ti) { rem -= p.NT - ti; ++ti; }
    const int tj = ti + rem;
    const int f = (int)(bin % p.n_freq), grp = (int)(bin / p.n_freq);
    const T2* Xb = X + (int64_t)f * p.a.sF + sc_group_offset(p.a, grp);
    const int C = p.a.C;
    const ScRec rec = p.total + bin * p.rec_stride;
    const bool want_pow = p.measures & SC_JACKKNIFE_POWER, want_coh = p.measures & SC_JACKKNIFE_COHERENCE_MAGNITUDE,
               want_im = p.measures & SC_JACKKNIFE_IMAGINARY_COHERENCE;
    const bool diag_thread = ti == tj && tx == ty;
    const double nan = __builtin_nan("");

    int ci[2], cj[2];
    double Sii[2], Sjj[2], Sre[2][2], Sim[2][2], bcoh[2][2], bim[2][2];
    bool valid[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        double dummy;
        ci[a] = ti * JK_T + ty + 16 * a;
        cj[a] = tj * JK_T + tx + 16 * a;
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
            if (++cnt == p.g) {
                // the unit is complete: d_u = theta(S - G_u) - theta(S) of every measure, in fp64
                cnt = 0;
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
                                // atanh(x) - atanh(y) = atanh((x - y) / (1 - x y)): no difference of two nearly equal transcendentals
                                const double mag = sqrt(re * re + im * im) * rr;
                                const double d = atanh((mag - bcoh[a][b]) / (1.0 - mag * bcoh[a][b]));
                                coh1[a][b] += d;
                                coh2[a][b] += d * d;
                            }
                            if (want_im) {
                                const double d = im * rr - bim[a][b];
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
                        const double d = log1p(-(double)Pi[a] / Sii[a]) + p.ln_ratio;
                        pw1[a] += d;
                        pw2[a] += d * d;
                    }
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) { Pi[a] = 0; Pj[a] = 0; }
            }
        }
    }

    double* out = p.out + (int64_t)blockIdx.y * p.out_doubles;
    const int64_t CC = (int64_t)C * C, plane2 = p.n_bins * CC;
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
                const int64_t plane1 = p.n_bins * C;
                th[ci[a]] = Sii[a] > 0.0 ? log(Sii[a] / (p.n_total * (double)p.g)) : nan;
                th[plane1 + ci[a]] = Sii[a] > 0.0 ? pw1[a] : nan;
                th[2 * plane1 + ci[a]] = Sii[a] > 0.0 ? pw2[a] : nan;
            }
        }
    }
}

// partial sums of the unit splits -> the output, in split order; theta(S) is the same in every split
__global__ void jk_fold(const double* __restrict__ ws, int n_splits, JkArgs p, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.out_doubles) return;
    bool is_theta = false;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (p.off[m] < 0) continue;
        const int64_t len = p.n_bins * (m == 0 ? (int64_t)p.a.C : (int64_t)p.a.C * p.a.C);
        if (e >= p.off[m] && e < p.off[m] + len) is_theta = true;
    }
    double v = ws[e];
    if (!is_theta)
        for (int s = 1; s < n_splits; ++s) v += ws[(int64_t)s * p.out_doubles + e];
    out[e] = v;
}

struct JkPlan {
    ScAxes a;
    int64_t n_bins, n_units, g, out_doubles, off[3];
    int NT, n_tp, q_tapers;
};

int jk_plan(const sc_spectra_desc* desc, uint32_t measures, int over, JkPlan* pl) {
    SC_REQUIRE(desc, "NULL descriptor");
    if (sc_make_axes(desc, &pl->a) != SC_OK) return SC_EINVAL;
    const ScAxes& a = pl->a;
    SC_REQUIRE(a.F >= 1 && a.W >= 1 && a.R >= 1 && a.K >= 1 && a.C >= 1 && a.C <= 32768, "bad spectra sizes");
    SC_REQUIRE(measures && !(measures & ~(SC_JACKKNIFE_POWER | SC_JACKKNIFE_COHERENCE_MAGNITUDE | SC_JACKKNIFE_IMAGINARY_COHERENCE)),
               "measures: a non-empty mask of SC_JACKKNIFE_POWER, _COHERENCE_MAGNITUDE, _IMAGINARY_COHERENCE");
    SC_REQUIRE(over == SC_JACKKNIFE_OVER_TRIALS || over == SC_JACKKNIFE_OVER_OBSERVATIONS, "over: SC_JACKKNIFE_OVER_TRIALS or _OBSERVATIONS");
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
    for (int m = 0; m < 3; ++m) {
        pl->off[m] = -1;
        if (measures & (1u << m)) {
            pl->off[m] = at;
            at += 3 * pl->n_bins * (m == 0 ? (int64_t)a.C : (int64_t)a.C * a.C);
        }
    }
    pl->out_doubles = at;
    return SC_OK;
}

// units per split and number of splits: only when bins x tile pairs leave compute units idle, and never fewer than 16 units each
void jk_splits(const JkPlan& pl, int64_t n_local, int64_t* per, int64_t* n_splits) {
    const int64_t base = pl.n_bins * pl.n_tp;
    int64_t want = base >= 1024 ? 1 : (2048 + base - 1) / base;
    const int64_t by_units = n_local / 16 > 1 ? n_local / 16 : 1;
    if (want > by_units) want = by_units;
    if (want > JK_MAX_SPLITS) want = JK_MAX_SPLITS;
    *per = (n_local + want - 1) / want;
    *n_splits = (n_local + *per - 1) / *per;
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
    SC_REQUIRE(0 <= unit_begin && unit_begin < unit_end && unit_end <= pl.n_units, "unit range outside the spectra's units");
    SC_REQUIRE(n_units_total >= 2 && n_units_total >= unit_end - unit_begin, "a jackknife needs at least two units");
    int64_t per, n_splits;
    jk_splits(pl, unit_end - unit_begin, &per, &n_splits);
    SC_REQUIRE(per * pl.g < (int64_t)1 << 31, "too many observation rows per workgroup");
    if (n_splits > 1)
        SC_REQUIRE(d_workspace && workspace_bytes >= n_splits * pl.out_doubles * (int64_t)sizeof(double), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    JkArgs p = {};
    p.a = pl.a;
    p.total = sc_rec(d_total, planes);
    p.NB16 = sc_n_blocks(pl.a.C);
    p.n_tiles16 = sc_n_tiles(p.NB16);
    p.p_csm = sc_plane_offset(planes, SC_PLANE_CSM);
    p.rec_stride = (int64_t)sc_plane_count(planes) * p.n_tiles16 * SC_TILE_ELEMS;
    p.n_freq = pl.a.F; p.NT = pl.NT; p.n_tp = pl.n_tp;
    p.over = over; p.g = (int)pl.g; p.q_tapers = pl.q_tapers;
    p.unit_begin = unit_begin; p.unit_end = unit_end; p.units_per_split = per;
    p.n_total = (double)n_units_total;
    p.ln_ratio = log((double)n_units_total / (double)(n_units_total - 1));
    p.measures = measures;
    p.n_bins = pl.n_bins;
    for (int m = 0; m < 3; ++m) p.off[m] = pl.off[m];
    p.out_doubles = pl.out_doubles;
    p.out = n_splits > 1 ? (double*)d_workspace : d_out;
    const dim3 grid((unsigned)(pl.n_bins * pl.n_tp), (unsigned)n_splits);
    hipLaunchKernelGGL((jk_kernel<T, T2>), grid, dim3(256), 0, st, (const T2*)d_X, p);
    SC_CHECK_HIP(hipGetLastError());
    if (n_splits > 1) {
        hipLaunchKernelGGL(jk_fold, dim3((unsigned)((pl.out_doubles + 255) / 256)), dim3(256), 0, st, (const double*)d_workspace,
                           (int)n_splits, p, d_out);
        SC_CHECK_HIP(hipGetLastError());
    }
    return SC_OK;
}

}  // namespace

extern "C" int sc_jackknife_layout(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t* n_bins, int64_t* n_units,
                                   int64_t* unit_size, int64_t* out_doubles) {
    JkPlan pl;
    const int rc = jk_plan(desc, measures, over, &pl);
    if (rc != SC_OK) return rc;
    if (n_bins) *n_bins = pl.n_bins;
    if (n_units) *n_units = pl.n_units;
    if (unit_size) *unit_size = pl.g;
    if (out_doubles) *out_doubles = pl.out_doubles;
    return SC_OK;
}

extern "C" int64_t sc_jackknife_workspace_bytes(const sc_spectra_desc* desc, uint32_t measures, int over, int64_t unit_begin,
                                                int64_t unit_end) {
    JkPlan pl;
    if (jk_plan(desc, measures, over, &pl) != SC_OK || unit_end <= unit_begin) return 0;
    int64_t per, n_splits;
    jk_splits(pl, unit_end - unit_begin, &per, &n_splits);
    return n_splits > 1 ? n_splits * pl.out_doubles * (int64_t)sizeof(double) : 0;
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
