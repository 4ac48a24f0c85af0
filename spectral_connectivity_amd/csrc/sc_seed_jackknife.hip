// sc_seed_jackknife.hip -- delete-one jackknife of seed-based connectivity: a few signals (seeds) against a list of signals
// (targets), for the coherency pair and the phase-lag family in one walk over the spectra (gfx950).
//
// The statistic is that of sc_jackknife.hip (d_u = theta(total - unit) - theta(total); theta, sum d, sum d^2 out; the host finishes),
// the entries and the record those of sc_seed.hip (s = x_seed conj(x_target); double [bin][plane][n_seeds][n_targets], then the power
// sums).  Neither kernel's geometry carries over: the seed kernel's waves split the rows of a block, so a unit's rows land in
// different waves, and the all-pairs walk owns a square of channel tiles.
//
// sjk_kernel.  One workgroup of 256 threads owns (bin, tile of targets, chunk of seeds, share of the units); a thread owns ONE entry
// (seed, target), so all it carries -- 7 unit sums, 7 totals, pivot / sum d / sum d^2 of six measures -- lives in registers whatever
// the measures.  The four waves are `cw` seeds x 4 / cw parts of 64 targets: cw = 4 (tile of 64 targets), or 2 (tile of 128) for a
// request of two seeds, where it is measurably faster; 1 (tile of 256) exists for measurements only
// (SjkPlan).  All four waves stage a block of 2048 target coefficients in LDS -- 32 * cw / 4 rows of the tile, a wave's load being 512
// (1024: complex128) contiguous bytes of a row where the targets are ascending, 8 loads in flight per thread -- and the chunk's seed
// coefficients of those rows; the row offsets are decoded once per block.  Every wave then reads the block's rows of its 64 targets
// lane-contiguously and its seed's coefficient as a broadcast, adds the row to the unit sums and, after a unit's g-th row, calls the
// unit step.  A unit may straddle blocks: what is carried is in registers.  Seed chunks, then target tiles, then bins are consecutive
// workgroups, so a bin's rows come from HBM once and from cache for the others.  Where bins x tiles x chunks do not fill the chip
// the units are split over gridDim.y workgroups of at least 16 units that write partial sums to the workspace, added in split order
// by sjk_fold: no floating-point atomics, bit-identical results from run to run.
//
// The unit sums (SjkUnit), in the spectra's precision: Re s, Im s, |Im s|, (Im s)^2, sign(Im s) (an integer), |x_seed|^2, |x_target|^2.
// TOTALS = true: the unit step adds them to seven fp64 sums, written as a seed record with the planes asked for -- each total is by
// construction the fp64 sum of the very unit sums the other instantiation subtracts from it (the seed
// accumulator's own record groups a wave's rows differently, and the debiased wPLI^2 multiplies the mismatch by B / |A|).
// TOTALS = false: the unit step forms d_u of every requested measure in fp64 (sc_jackknife_value.h: the formulas of the all-pairs
// kernels) and adds it to the sums about the first unit's deviation, moved back to the origin after the last unit.  The measure mask
// is a wave-uniform run-time argument.
#include "sc_jackknife_value.h"
#include "sc_seed_layout.h"
#include "sc_workspace.h"

#include <stdlib.h>

namespace {

constexpr int SJK_ELEMS = 2048;           // target coefficients of a staging block: 32 rows x 64 ... 8 rows x 256
constexpr int SJK_LOADS = SJK_ELEMS / 256;
constexpr int SJK_MAX_ROWS = 32;
constexpr int SJK_MAX_SPLITS = 256;
constexpr int SJK_MEASURES = 6;
constexpr uint32_t SJK_ALL = SC_SEED_JACKKNIFE_COHERENCE_MAGNITUDE | SC_SEED_JACKKNIFE_IMAGINARY_COHERENCE | SC_SEED_JACKKNIFE_PLI |
                             SC_SEED_JACKKNIFE_WPLI | SC_SEED_JACKKNIFE_DEBIASED_PLI2 | SC_SEED_JACKKNIFE_DEBIASED_WPLI2;
constexpr uint32_t SJK_PLANES_ALL = SC_PLANE_CSM | SC_PLANE_ABS_IM | SC_PLANE_IM_SQ | SC_PLANE_SIGN_IM | SC_SEED_PLANE_POWER;

struct SjkArgs {
    ScAxes a;
    const int32_t* seeds;
    const int32_t* targets;      // nullptr: target t is signal t
    int n_seeds, n_targets, n_chunks, n_tiles;
    int cw;                      // seeds of a workgroup: 1, 2 or 4 (4 / cw parts of 64 targets each)
    int over, g, q_tapers;       // rows per unit; tapers per window inside a unit (over = trials)
    int64_t unit_begin, unit_end, units_per_split;
    int64_t n_bins;
    SeedLayout l;                // of the record: the totals read (TOTALS = false) or written
    const double* total;
    double n_full, n_del;        // observations of the full estimate and of a delete-one estimate
    uint32_t measures;
    int64_t off[SJK_MEASURES];   // first double of each measure's block, -1: not requested
    int64_t out_doubles;         // of one split: the measure blocks, or the record
    double* out;                 // split y writes at out + y * out_doubles
};

// the sums of one unit for a thread's entry, in the engine's precision: what the jackknife subtracts from the totals and what the
// totals pass adds up to them
template <typename T>
struct SjkUnit {
    T re, im, ab, sq, ps, pt;    // sum Re s, Im s, |Im s|, (Im s)^2, |x_seed|^2, |x_target|^2
    int sg;                      // sum sign(Im s)

    __device__ __forceinline__ void clear() { re = 0; im = 0; ab = 0; sq = 0; ps = 0; pt = 0; sg = 0; }
    template <typename T2>
    __device__ __forceinline__ void add(const T2 y, const T2 x) {          // y: the seed's coefficient, x: the target's
        const T i = y.y * x.x - y.x * x.y;
        re += y.x * x.x + y.y * x.y;
        im += i;
        ab += i < 0 ? -i : i;
        sq += i * i;
        sg += (i > 0) - (i < 0);
        ps += y.x * y.x + y.y * y.y;
        pt += x.x * x.x + x.y * x.y;
    }
};

template <typename T, typename T2, bool TOTALS>
__global__ __launch_bounds__(256) void sjk_kernel(const T2* __restrict__ X, SjkArgs p) {
    __shared__ T2 rows[SJK_ELEMS];                    // [rows of the block][targets of the tile]
    __shared__ T2 sx[SJK_MAX_ROWS * 4];               // [rows of the block][seeds of the chunk]
    __shared__ int64_t row_off[SJK_MAX_ROWS];         // element offset of every staged row: one decode per row
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = p.cw, parts = 4 / cw, TW = SEED_TILE * parts, RB = SJK_ELEMS / TW;
    int64_t wg = blockIdx.x;
    const int chunk = (int)(wg % p.n_chunks); wg /= p.n_chunks;
    const int tile = (int)(wg % p.n_tiles);
    const int64_t bin = wg / p.n_tiles;
    const int f = (int)(bin % p.a.F), grp = (int)(bin / p.a.F);
    const T2* Xb = X + (int64_t)f * p.a.sF + sc_group_offset(p.a, grp);
    const int C = p.a.C;
    const int s0 = chunk * cw;
    const int ns = p.n_seeds - s0 < cw ? p.n_seeds - s0 : cw;

    // this thread's entry: seed `slot` of the chunk (wave-uniform) against target t; a wave without a seed only stages, a lane past
    // the target list computes on zeros and stores nothing
    const int slot = wave / parts, part = wave - slot * parts;
    const bool active = slot < ns;
    const int s = s0 + slot;
    const int t = tile * TW + part * SEED_TILE + lane;
    const bool t_in = t < p.n_targets;
    int ct = -1, cs = -2;
    if (t_in) ct = p.targets ? p.targets[t] : t;
    if (active) cs = p.seeds[s];

    // what this thread stages: column st_col of the tile in the rows st_r0 + cw k, and (threads 0 .. RB cw - 1) seed sd_s of row sd_r.
    // An index outside [0, C) loads nothing and counts as a signal of zeros.
    const int st_col = tid & (TW - 1), st_r0 = tid / TW;
    int st_c = -1;
    if (tile * TW + st_col < p.n_targets) st_c = p.targets ? p.targets[tile * TW + st_col] : tile * TW + st_col;
    const bool st_ok = (unsigned)st_c < (unsigned)C;
    const int sd_r = tid / cw, sd_s = tid - sd_r * cw;
    int sd_c = -1;
    if (tid < RB * cw && sd_s < ns) sd_c = p.seeds[s0 + sd_s];
    const bool sd_ok = (unsigned)sd_c < (unsigned)C;

    const int64_t u0 = p.unit_begin + (int64_t)blockIdx.y * p.units_per_split;
    const int64_t u1 = u0 + p.units_per_split < p.unit_end ? u0 + p.units_per_split : p.unit_end;
    const int n_rows = (int)((u1 - u0) * p.g);

    const bool want_coh = p.measures & SC_SEED_JACKKNIFE_COHERENCE_MAGNITUDE, want_im = p.measures & SC_SEED_JACKKNIFE_IMAGINARY_COHERENCE,
               want_pli = p.measures & SC_SEED_JACKKNIFE_PLI, want_wpli = p.measures & SC_SEED_JACKKNIFE_WPLI,
               want_dpli = p.measures & SC_SEED_JACKKNIFE_DEBIASED_PLI2, want_dwpli = p.measures & SC_SEED_JACKKNIFE_DEBIASED_WPLI2;
    const int64_t cells = (int64_t)p.n_seeds * p.n_targets;
    const int64_t e = (int64_t)s * p.n_targets + t;       // this entry in a [n_seeds][n_targets] block
    const bool stores = active && t_in;

    // the totals: summed here (TOTALS), or read from the record
    double tRe = 0.0, tA = 0.0, tB = 0.0, tQ = 0.0, tN = 0.0, tPs = TOTALS ? 0.0 : 1.0, tPt = TOTALS ? 0.0 : 1.0;
    double th[SJK_MEASURES] = {};                           // the full estimates (the coherence magnitude before atanh)
    if (!TOTALS && stores) {
        const double* rec = p.total + bin * p.l.per_bin;
        if (p.l.p_csm >= 0) { tRe = rec[p.l.p_csm * cells + e]; tA = rec[(p.l.p_csm + 1) * cells + e]; }
        if (p.l.p_abs >= 0) tB = rec[p.l.p_abs * cells + e];
        if (p.l.p_sq >= 0) tQ = rec[p.l.p_sq * cells + e];
        if (p.l.p_sign >= 0) tN = rec[p.l.p_sign * cells + e];
        if (p.l.pow_off >= 0) { tPs = rec[p.l.pow_off + s]; tPt = rec[p.l.pow_off + p.n_seeds + t]; }
    }
    if (!TOTALS) {
        const double rr = (1.0 / sqrt(tPs)) * (1.0 / sqrt(tPt));
        th[0] = sqrt(tRe * tRe + tA * tA) * rr;
        th[1] = tA * rr;
        const double pli = jk_pli(tN, p.n_full);
        th[2] = pli;
        th[3] = jk_wpli(tA, tB, p.n_full);
        th[4] = jk_debiased_pli2(pli, p.n_full);
        th[5] = jk_debiased_wpli2(tA, tB, tQ);
    }

    double s1[SJK_MEASURES] = {}, s2[SJK_MEASURES] = {}, piv[SJK_MEASURES] = {};
    int n_done = 0, cnt = 0;
    SjkUnit<T> u;
    u.clear();

    for (int r0 = 0; r0 < n_rows; r0 += RB) {
        const int nr = n_rows - r0 < RB ? n_rows - r0 : RB;
        __syncthreads();
        if (tid < nr) {
            const int q = r0 + tid, du = q / p.g;
            row_off[tid] = jk_unit_row_offset(p.a, p.over, p.q_tapers, u0 + du, q - du * p.g);
        }
        __syncthreads();
        T2 xt[SJK_LOADS], xs;
        xs.x = 0; xs.y = 0;
        if (sd_ok && sd_r < nr) xs = Xb[row_off[sd_r] + sd_c];
#pragma unroll
        for (int k = 0; k < SJK_LOADS; ++k) {
            const int r = st_r0 + cw * k;
            xt[k].x = 0; xt[k].y = 0;
            if (st_ok && r < nr) xt[k] = Xb[row_off[r] + st_c];
        }
        if (tid < RB * cw) sx[tid] = xs;
#pragma unroll
        for (int k = 0; k < SJK_LOADS; ++k) rows[(st_r0 + cw * k) * TW + st_col] = xt[k];
        __syncthreads();
        if (!active) continue;
        for (int r = 0; r < nr; ++r) {
            u.add(sx[r * cw + slot], rows[r * TW + part * SEED_TILE + lane]);
            if (++cnt < p.g) continue;
            cnt = 0;
            // the unit is complete
            if (TOTALS) {
                tRe += (double)u.re; tA += (double)u.im; tB += (double)u.ab; tQ += (double)u.sq; tN += (double)u.sg;
                tPs += (double)u.ps; tPt += (double)u.pt;
            } else {
                // d_u = theta(totals without the unit, n') - theta(totals, n) of every requested measure, in fp64
                const bool first = n_done == 0;
                const double A = tA - (double)u.im;
                if (want_coh || want_im) {
                    const double rr = (1.0 / sqrt(tPs - (double)u.ps)) * (1.0 / sqrt(tPt - (double)u.pt));
                    if (want_coh) {
                        const double re = tRe - (double)u.re;
                        jk_shifted_add(jk_fisher_deviation(sqrt(re * re + A * A) * rr, th[0]), first, piv[0], s1[0], s2[0]);
                    }
                    if (want_im) jk_shifted_add(jk_imaginary_deviation(A, rr, th[1]), first, piv[1], s1[1], s2[1]);
                }
                if (want_pli || want_dpli) {
                    const double pli = jk_pli(tN - (double)u.sg, p.n_del);
                    if (want_pli) jk_shifted_add(pli - th[2], first, piv[2], s1[2], s2[2]);
                    if (want_dpli) jk_shifted_add(jk_debiased_pli2(pli, p.n_del) - th[4], first, piv[4], s1[4], s2[4]);
                }
                if (want_wpli || want_dwpli) {
                    const double B = tB - (double)u.ab;
                    if (want_wpli) jk_shifted_add(jk_wpli(A, B, p.n_del) - th[3], first, piv[3], s1[3], s2[3]);
                    if (want_dwpli) jk_shifted_add(jk_debiased_wpli2(A, B, tQ - (double)u.sq) - th[5], first, piv[5], s1[5], s2[5]);
                }
                ++n_done;
            }
            u.clear();
        }
    }

    double* out = p.out + (int64_t)blockIdx.y * p.out_doubles;
    if (TOTALS) {
        double* rec = out + bin * p.l.per_bin;
        if (stores) {
            if (p.l.p_csm >= 0) { rec[p.l.p_csm * cells + e] = tRe; rec[(p.l.p_csm + 1) * cells + e] = tA; }
            if (p.l.p_abs >= 0) rec[p.l.p_abs * cells + e] = tB;
            if (p.l.p_sq >= 0) rec[p.l.p_sq * cells + e] = tQ;
            if (p.l.p_sign >= 0) rec[p.l.p_sign * cells + e] = tN;
            if (p.l.pow_off >= 0) {
                // the powers once per bin: a seed's from the first target of tile 0, a target's from the first seed of chunk 0
                if (tile == 0 && part == 0 && lane == 0) rec[p.l.pow_off + s] = tPs;
                if (chunk == 0 && slot == 0) rec[p.l.pow_off + p.n_seeds + t] = tPt;
            }
        }
        return;
    }
    if (!stores) return;
    const bool diag = cs == ct;                           // a seed that is its own target: the jackknife's diagonal
    const double nan = __builtin_nan("");
    th[0] = atanh(th[0]);
    const int64_t len = p.n_bins * cells;
#pragma unroll
    for (int m = 0; m < SJK_MEASURES; ++m) {
        if (p.off[m] < 0) continue;
        jk_shifted_finish(n_done, piv[m], s1[m], s2[m]);
        double* o = out + p.off[m] + bin * cells + e;
        o[0] = diag ? nan : th[m];
        o[len] = diag ? nan : s1[m];
        o[2 * len] = diag ? nan : s2[m];
    }
}

// partial sums of the unit splits -> the output, in split order.  theta_len > 0: the output is blocks of three arrays of theta_len
// doubles -- theta, sum d, sum d^2 -- and theta is the same in every split; 0: every double is a sum over the splits (a record).
__global__ void sjk_fold(const double* __restrict__ ws, int n_splits, int64_t out_doubles, int64_t theta_len, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= out_doubles) return;
    double v = ws[e];
    if (!(theta_len > 0 && (e / theta_len) % 3 == 0))
        for (int s = 1; s < n_splits; ++s) v += ws[(int64_t)s * out_doubles + e];
    out[e] = v;
}

// planes of the total record a mask of measures reads
uint32_t sjk_planes(uint32_t measures) {
    uint32_t need = 0;
    if (measures & (SC_SEED_JACKKNIFE_COHERENCE_MAGNITUDE | SC_SEED_JACKKNIFE_IMAGINARY_COHERENCE)) need |= SC_PLANE_CSM | SC_SEED_PLANE_POWER;
    if (measures & (SC_SEED_JACKKNIFE_PLI | SC_SEED_JACKKNIFE_DEBIASED_PLI2)) need |= SC_PLANE_SIGN_IM;
    if (measures & SC_SEED_JACKKNIFE_WPLI) need |= SC_PLANE_CSM | SC_PLANE_ABS_IM;
    if (measures & SC_SEED_JACKKNIFE_DEBIASED_WPLI2) need |= SC_PLANE_CSM | SC_PLANE_ABS_IM | SC_PLANE_IM_SQ;
    return need;
}

// One description of a call -- the geometry, the units, the output of one split and the unit splits of a range: the queries size the
// workspace from it and the launcher carves the workspace with it.
struct SjkPlan {
    ScAxes a;
    int n_seeds, n_targets, cw, n_chunks, n_tiles;
    int over, q_tapers;
    int64_t n_bins, n_units, g;
    int64_t off[SJK_MEASURES], theta_len, out_doubles;
    int64_t units_per_split, n_splits;                   // of the range given to sjk_split
};

// seeds of a workgroup.  Every wave owns one (seed, 64 targets): 4 seeds x 64 targets, except for a request of two seeds -- the
// headline shape --, where two of the four waves would only stage: 2 seeds x 128 targets is measurably faster there (all six
// measures of 2 seeds against 308 signals: 18.1 ms against 19.6 on complex64 spectra, 24.7 against 30.4 on complex128;
// profiles/seed_jackknife_time.txt).  One seed keeps 4 x 64: 1 x 256 has not been timed on a request of one
// seed.  The diagnostic switch SC_SEED_JACKKNIFE_CHUNK = 1, 2, 4 (sc_switch: the library's snapshot of the environment, the same in
// the workspace query and in the launch) overrides the choice for such measurements.
int sjk_chunk_width(int64_t n_seeds) {
    if (const char* v = sc_switch(SC_SW_SEED_JACKKNIFE_CHUNK)) {
        const int w = atoi(v);
        if (w == 1 || w == 2 || w == 4) return w;
    }
    return n_seeds == 2 ? 2 : 4;
}

// measures != 0: a jackknife call with that mask; 0: a totals call writing a record with `planes`
int sjk_plan(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t measures, uint32_t planes, int over, SjkPlan* pl) {
    SC_REQUIRE(desc, "NULL descriptor");
    if (sc_make_axes(desc, &pl->a) != SC_OK) return SC_EINVAL;
    const ScAxes& a = pl->a;
    SC_REQUIRE(a.F >= 1 && a.W >= 1 && a.R >= 1 && a.K >= 1 && a.C >= 1 && a.C <= 32768, "bad spectra sizes");
    const int rc = seed_check_counts(n_seeds, n_targets, planes);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(!(planes & ~SJK_PLANES_ALL), "planes: a set of SC_PLANE_CSM, _ABS_IM, _IM_SQ, _SIGN_IM and SC_SEED_PLANE_POWER");
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
    pl->n_seeds = (int)n_seeds; pl->n_targets = (int)n_targets;
    pl->cw = sjk_chunk_width(n_seeds);
    const int tile = SEED_TILE * (4 / pl->cw);
    pl->n_chunks = (pl->n_seeds + pl->cw - 1) / pl->cw;
    pl->n_tiles = (pl->n_targets + tile - 1) / tile;
    pl->n_bins = (int64_t)a.n_groups * a.F;
    SC_REQUIRE(pl->n_bins * pl->n_tiles * pl->n_chunks < (int64_t)1 << 31, "too many (bin, target tile, seed chunk) workgroups for one launch");
    pl->theta_len = pl->n_bins * n_seeds * n_targets;
    int64_t at = 0;
    for (int m = 0; m < SJK_MEASURES; ++m) {
        pl->off[m] = -1;
        if (measures & (1u << m)) {
            pl->off[m] = at;
            at += 3 * pl->theta_len;
        }
    }
    if (!measures) {
        pl->theta_len = 0;
        at = pl->n_bins * seed_layout(pl->n_seeds, pl->n_targets, planes).per_bin;
    }
    pl->out_doubles = at;
    pl->units_per_split = pl->n_splits = 0;
    return SC_OK;
}

int sjk_jackknife_plan(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t measures, int over, SjkPlan* pl) {
    SC_REQUIRE(measures && !(measures & ~SJK_ALL),
               "measures: a non-empty mask of SC_SEED_JACKKNIFE_COHERENCE_MAGNITUDE, _IMAGINARY_COHERENCE, _PLI, _WPLI, _DEBIASED_PLI2, "
               "_DEBIASED_WPLI2");
    return sjk_plan(desc, n_seeds, n_targets, measures, sjk_planes(measures), over, pl);
}

// the unit range of a call against the plan's units, and its splits
int sjk_split(SjkPlan* pl, int64_t unit_begin, int64_t unit_end) {
    SC_REQUIRE(0 <= unit_begin && unit_begin < unit_end && unit_end <= pl->n_units, "unit range outside the spectra's units");
    jk_unit_splits(pl->n_bins * pl->n_tiles * pl->n_chunks, unit_end - unit_begin, SJK_MAX_SPLITS, &pl->units_per_split, &pl->n_splits);
    SC_REQUIRE(pl->units_per_split * pl->g < (int64_t)1 << 31, "too many observation rows per workgroup");
    return SC_OK;
}

struct SjkWorkspace { double* partial; };
SjkWorkspace sjk_workspace(ScCarver& w, const SjkPlan& pl) {
    SjkWorkspace k;
    k.partial = w.take<double>("partial sums", pl.n_splits > 1 ? (size_t)(pl.n_splits * pl.out_doubles) : 0, 16);
    return k;
}

// bytes the splits of a unit range need (0: one split, no workspace; 0 too where the plan or the range failed)
int64_t sjk_workspace_bytes(int plan_rc, SjkPlan* pl, int64_t unit_begin, int64_t unit_end) {
    if (plan_rc != SC_OK || sjk_split(pl, unit_begin, unit_end) != SC_OK) return 0;
    ScCarver need(nullptr);
    sjk_workspace(need, *pl);
    return (int64_t)need.used;
}

// What the two entry points share once the plan stands and their own checks have passed: the workspace, the launch, the fold.
template <typename T, typename T2, bool TOTALS>
int sjk_launch(const SjkPlan& pl, SjkArgs* p, const void* d_X, double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    ScCarver need(nullptr);
    sjk_workspace(need, pl);
    SC_REQUIRE(need.used == 0 || (d_workspace && workspace_bytes >= (int64_t)need.used), "workspace too small");
    SC_REQUIRE((uintptr_t)d_workspace % 16 == 0, "workspace must be 16-byte aligned");
    ScCarver carve(d_workspace);
    const SjkWorkspace ws = sjk_workspace(carve, pl);
    p->a = pl.a;
    p->n_seeds = pl.n_seeds; p->n_targets = pl.n_targets; p->n_chunks = pl.n_chunks; p->n_tiles = pl.n_tiles; p->cw = pl.cw;
    p->over = pl.over; p->g = (int)pl.g; p->q_tapers = pl.q_tapers;
    p->units_per_split = pl.units_per_split;
    p->n_bins = pl.n_bins;
    for (int m = 0; m < SJK_MEASURES; ++m) p->off[m] = pl.off[m];
    p->out_doubles = pl.out_doubles;
    p->out = pl.n_splits > 1 ? ws.partial : d_out;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(pl.n_bins * pl.n_tiles * pl.n_chunks), (unsigned)pl.n_splits);
    hipLaunchKernelGGL((sjk_kernel<T, T2, TOTALS>), grid, dim3(256), 0, st, (const T2*)d_X, *p);
    SC_CHECK_HIP(hipGetLastError());
    if (pl.n_splits > 1) {
        hipLaunchKernelGGL(sjk_fold, dim3((unsigned)((pl.out_doubles + 255) / 256)), dim3(256), 0, st, (const double*)ws.partial,
                           (int)pl.n_splits, pl.out_doubles, pl.theta_len, d_out);
        SC_CHECK_HIP(hipGetLastError());
    }
    return SC_OK;
}

template <typename T, typename T2>
int sjk_totals_run(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds, const int32_t* d_targets,
                   int64_t n_targets, uint32_t planes, int over, int64_t unit_begin, int64_t unit_end, double* d_record,
                   void* d_workspace, int64_t workspace_bytes, void* stream) {
    ScTimed timed_("seed_jackknife_totals", stream);
    SjkPlan pl;
    int rc = sjk_plan(desc, n_seeds, n_targets, 0, planes, over, &pl);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(d_X && d_seeds && d_record, "NULL argument");
    if ((rc = sjk_split(&pl, unit_begin, unit_end)) != SC_OK) return rc;
    SjkArgs p = {};
    p.seeds = d_seeds; p.targets = d_targets;
    p.unit_begin = unit_begin; p.unit_end = unit_end;
    p.l = seed_layout(pl.n_seeds, pl.n_targets, planes);
    return sjk_launch<T, T2, true>(pl, &p, d_X, d_record, d_workspace, workspace_bytes, stream);
}

template <typename T, typename T2>
int sjk_run(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds, const int32_t* d_targets,
            int64_t n_targets, const double* d_total, uint32_t planes, uint32_t measures, int over, int64_t unit_begin,
            int64_t unit_end, int64_t n_units_total, double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    ScTimed timed_("seed_jackknife", stream);
    SjkPlan pl;
    int rc = sjk_jackknife_plan(desc, n_seeds, n_targets, measures, over, &pl);
    if (rc != SC_OK) return rc;
    SC_REQUIRE(d_X && d_seeds && d_total && d_out, "NULL argument");
    if ((rc = seed_check_counts(n_seeds, n_targets, planes)) != SC_OK) return rc;
    SC_REQUIRE(!(planes & ~SJK_PLANES_ALL), "planes: a set of SC_PLANE_CSM, _ABS_IM, _IM_SQ, _SIGN_IM and SC_SEED_PLANE_POWER");
    const uint32_t need = sjk_planes(measures);
    SC_REQUIRE((planes & need) == need,
               "the total record lacks a plane of a requested measure (coherence magnitude, imaginary coherence: SC_PLANE_CSM | "
               "SC_SEED_PLANE_POWER; PLI, debiased PLI^2: SC_PLANE_SIGN_IM; wPLI: SC_PLANE_CSM | _ABS_IM; debiased wPLI^2: SC_PLANE_CSM | "
               "_ABS_IM | _IM_SQ)");
    if ((rc = sjk_split(&pl, unit_begin, unit_end)) != SC_OK) return rc;
    SC_REQUIRE(n_units_total >= 2 && n_units_total >= unit_end - unit_begin, "a jackknife needs at least two units");
    if (measures & (SC_SEED_JACKKNIFE_DEBIASED_PLI2 | SC_SEED_JACKKNIFE_DEBIASED_WPLI2))
        SC_REQUIRE((n_units_total - 1) * pl.g >= 2, "a debiased estimate needs at least two observations in a delete-one set");
    SjkArgs p = {};
    p.seeds = d_seeds; p.targets = d_targets;
    p.unit_begin = unit_begin; p.unit_end = unit_end;
    p.l = seed_layout(pl.n_seeds, pl.n_targets, planes);
    p.total = d_total;
    p.n_full = (double)n_units_total * (double)pl.g;
    p.n_del = (double)(n_units_total - 1) * (double)pl.g;
    p.measures = measures;
    return sjk_launch<T, T2, false>(pl, &p, d_X, d_out, d_workspace, workspace_bytes, stream);
}

}  // namespace

extern "C" int sc_seed_jackknife_layout(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t measures, int over,
                                        int64_t* n_bins, int64_t* n_units, int64_t* unit_size, int64_t* out_doubles) {
    SjkPlan pl;
    const int rc = sjk_jackknife_plan(desc, n_seeds, n_targets, measures, over, &pl);
    if (rc != SC_OK) return rc;
    if (n_bins) *n_bins = pl.n_bins;
    if (n_units) *n_units = pl.n_units;
    if (unit_size) *unit_size = pl.g;
    if (out_doubles) *out_doubles = pl.out_doubles;
    return SC_OK;
}

extern "C" int64_t sc_seed_jackknife_workspace_bytes(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets, uint32_t measures,
                                                     int over, int64_t unit_begin, int64_t unit_end) {
    SjkPlan pl;
    return sjk_workspace_bytes(sjk_jackknife_plan(desc, n_seeds, n_targets, measures, over, &pl), &pl, unit_begin, unit_end);
}

extern "C" int64_t sc_seed_jackknife_totals_workspace_bytes(const sc_spectra_desc* desc, int64_t n_seeds, int64_t n_targets,
                                                            uint32_t planes, int over, int64_t unit_begin, int64_t unit_end) {
    SjkPlan pl;
    return sjk_workspace_bytes(sjk_plan(desc, n_seeds, n_targets, 0, planes, over, &pl), &pl, unit_begin, unit_end);
}

extern "C" int sc_seed_jackknife_totals_f32(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                            const int32_t* d_targets, int64_t n_targets, uint32_t planes, int over, int64_t unit_begin,
                                            int64_t unit_end, double* d_record, void* d_workspace, int64_t workspace_bytes,
                                            void* stream) {
    return sjk_totals_run<float, float2>(d_X, desc, d_seeds, n_seeds, d_targets, n_targets, planes, over, unit_begin, unit_end,
                                         d_record, d_workspace, workspace_bytes, stream);
}

extern "C" int sc_seed_jackknife_totals_f64(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                            const int32_t* d_targets, int64_t n_targets, uint32_t planes, int over, int64_t unit_begin,
                                            int64_t unit_end, double* d_record, void* d_workspace, int64_t workspace_bytes,
                                            void* stream) {
    return sjk_totals_run<double, double2>(d_X, desc, d_seeds, n_seeds, d_targets, n_targets, planes, over, unit_begin, unit_end,
                                           d_record, d_workspace, workspace_bytes, stream);
}

extern "C" int sc_seed_jackknife_f32(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                     const int32_t* d_targets, int64_t n_targets, const double* d_total, uint32_t planes,
                                     uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total,
                                     double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return sjk_run<float, float2>(d_X, desc, d_seeds, n_seeds, d_targets, n_targets, d_total, planes, measures, over, unit_begin,
                                  unit_end, n_units_total, d_out, d_workspace, workspace_bytes, stream);
}

extern "C" int sc_seed_jackknife_f64(const void* d_X, const sc_spectra_desc* desc, const int32_t* d_seeds, int64_t n_seeds,
                                     const int32_t* d_targets, int64_t n_targets, const double* d_total, uint32_t planes,
                                     uint32_t measures, int over, int64_t unit_begin, int64_t unit_end, int64_t n_units_total,
                                     double* d_out, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return sjk_run<double, double2>(d_X, desc, d_seeds, n_seeds, d_targets, n_targets, d_total, planes, measures, over, unit_begin,
                                    unit_end, n_units_total, d_out, d_workspace, workspace_bytes, stream);
}
