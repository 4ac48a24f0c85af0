// sc_jackknife_value.h -- what the delete-one jackknife kernels share (sc_jackknife.hip: all pairs; sc_seed_jackknife.hip: a few seeds
// against a list of targets): the statistics of the phase-lag family from the sums of a set of observations, the deviations of the
// coherency pair, the shifted sums, the rows of a delete unit and the split of the units over workgroups.  One copy, so that a seed
// entry and the all-pairs entry of the same two signals go through the same arithmetic.
#pragma once
#include "sc_common.h"

#include <math.h>

namespace {

// the four statistics from the sums (A, B, N, Q) of n observations; sc_measure.hip's formulas on the identity scale
__device__ __forceinline__ double jk_pli(double N, double n) { return N / n; }
__device__ __forceinline__ double jk_debiased_pli2(double pli, double n) { return (n * pli * pli - 1.0) / (n - 1.0); }
__device__ __forceinline__ double jk_wpli(double A, double B, double n) {
    double w = B / n;
    if (w < 2.220446049250313e-16) w = 1.0;
    return (A / n) / w;
}
__device__ __forceinline__ double jk_debiased_wpli2(double A, double B, double Q) {
    const double den = B * B - Q;
    return den == 0.0 ? __builtin_nan("") : (A * A - Q) / den;
}

// Fisher z of a delete-one coherence magnitude minus that of the full one: atanh(x) - atanh(y) = atanh((x - y) / (1 - x y)), no
// difference of two nearly equal transcendentals
__device__ __forceinline__ double jk_fisher_deviation(double mag, double full) { return atanh((mag - full) / (1.0 - mag * full)); }
// the imaginary coherence Im S / sqrt(S_ii S_jj) of a delete-one set (rr = 1 / sqrt(S_ii S_jj) of that set) minus the full one
__device__ __forceinline__ double jk_imaginary_deviation(double im, double rr, double full) { return im * rr - full; }

// one deviation into the two sums about the pivot (the first unit's deviation; see jk_phase_kernel)
__device__ __forceinline__ void jk_shifted_add(double d, bool first, double& piv, double& s1, double& s2) {
    if (first) piv = d;
    const double e = d - piv;
    s1 += e;
    s2 += e * e;
}
// the two sums of n_done deviations about the pivot r, moved back to the origin: sum d = k r + sum (d - r), sum d^2 = r sum d +
// sum (d - r)^2 + r sum (d - r)
__device__ __forceinline__ void jk_shifted_finish(int n_done, double piv, double& s1, double& s2) {
    const double r = piv, t1 = s1, t2 = s2;
    s1 = (double)n_done * r + t1;
    s2 = r * s1 + (t2 + r * t1);
}

// element offset of row q of delete unit u: over observations a unit is one observation; over trials it is the reduced windows x
// tapers of trial u, q_tapers tapers per window
__device__ __forceinline__ int64_t jk_unit_row_offset(const ScAxes& a, int over, int q_tapers, int64_t u, int q) {
    if (over == SC_JACKKNIFE_OVER_OBSERVATIONS) return sc_obs_offset(a, (int)u);
    const int w = q / q_tapers, k = q - w * q_tapers;
    return (int64_t)w * a.sW + u * a.sR + (int64_t)k * a.sK;
}

// units per split and number of splits of n_local units, for a launch of `base` workgroups per split: only when these leave
// compute units idle, never fewer than 16 units each, at most max_splits
inline void jk_unit_splits(int64_t base, int64_t n_local, int64_t max_splits, int64_t* per, int64_t* n_splits) {
    int64_t want = base >= 1024 ? 1 : (2048 + base - 1) / base;
    const int64_t by_units = n_local / 16 > 1 ? n_local / 16 : 1;
    if (want > by_units) want = by_units;
    if (want > max_splits) want = max_splits;
    *per = (n_local + want - 1) / want;
    *n_splits = (n_local + *per - 1) / *per;
}

}  // namespace
