// sc_measure_value.h -- the algebra of the expectation-type measures on the raw sums of one matrix entry: what the measures
// epilogue (sc_measure.hip) and the seed epilogue (sc_seed.hip) both evaluate.  Divides by n_observations (AFTER any cross-GPU
// sum) and applies the reference's algebra literally, in fp64:
//   coherency   connectivity.py:632-657   S_ij / max(sqrt(P_i P_j), eps), diagonal NaN
//   coherence   connectivity.py:675-702   clip(|coherency|^2, 0, 1)
//   imag. coh.  connectivity.py:704-743   clip(|Im S_ij| / max(sqrt(P_i P_j), eps), 0, 1)
//   PLV / PPC   connectivity.py:897-931, :1129-1159
//   PLI / wPLI / debiased  connectivity.py:933-1127  (Im forced to 0 on the diagonal)
#pragma once
#include <math.h>
#include "sc_common.h"

#define SC_EPS64 2.220446049250313e-16

// Products and sums are fused where one expression writes them, a * b + c, and nowhere else: the default lets the optimiser fuse
// what it finds after inlining, so the same measure_value rounded differently from one kernel instantiation to the next (PLV of a
// double record: the parts-summing one-launch kernel against the one-tile kernel, last bit).
#pragma clang fp contract(on)

// raw (un-normalised) sums of one matrix entry (i, j), as stored for the upper triangle
struct MeasureIn {
    double s_re, s_im;     // sum x_i conj(x_j)
    double p_i, p_j;       // sum |x_i|^2, sum |x_j|^2
    double sa, sq, sg;     // sum |Im s|, sum (Im s)^2, sum sign Im s
    double u_re, u_im;     // sum s / |s|
};

// the entry (j, i) from the sums of (i, j): s and the unit phasors are conjugated, sign Im s flips
__device__ inline MeasureIn measure_mirror(MeasureIn v) {
    MeasureIn w = v;
    w.s_im = -v.s_im; w.u_im = -v.u_im; w.sg = -v.sg; w.p_i = v.p_j; w.p_j = v.p_i;
    return w;
}

// 1 / x for a normal positive double: v_rcp_f64 and two Newton steps (<= 1 ulp; the IEEE division sequence is three times as long)
__device__ inline double measure_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// clip(x, 0, 1) and max(x, eps) as NumPy's: a NaN stays a NaN (fmin / fmax return their other argument, which turned the coherence
// of a non-finite channel into 0 or 1)
__device__ inline double measure_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
__device__ inline double measure_floor_eps(double x) { return x < SC_EPS64 ? SC_EPS64 : x; }

// one measure of one entry; complex measures return (re, im), real ones (value, 0)
__device__ inline double2 measure_value(int measure, double n, double rn, MeasureIn v, bool diag) {
    const double NaN = nan("");
    // (the expectation = sum * rn, rn = 1 / n from the host: no fp64 division per entry for it -- an fp64 division or square root is
    //  ~12-20 instructions at half rate, and they were HALF of this kernel's time: 0.131 ms for coherence + wPLI at cfg3 against 0.065 with
    //  the algebra switched off (-DMEASURE_AB_NOMATH); 1 ulp of fp64 apart from x / n)
    double s_re = v.s_re * rn, s_im = diag ? 0.0 : v.s_im * rn;
    const double p_i = v.p_i * rn, p_j = v.p_j * rn;
    switch (measure) {
    case SC_M_CSM:
        return make_double2(s_re, s_im);
    case SC_M_COHERENCY:
    case SC_M_COHERENCE_MAGNITUDE:
    case SC_M_COHERENCE_PHASE: {
        // 1 / max(sqrt(p_i p_j), eps) as ONE reciprocal square root (v_rsq_f64 + refinement) instead of a square root and a division
        const double pp = p_i * p_j;
        const double rden = pp <= SC_EPS64 * SC_EPS64 ? 1.0 / SC_EPS64 : rsqrt(pp);      // (a NaN product: NaN, like max(sqrt(NaN), eps))
        double c_re = s_re * rden, c_im = s_im * rden;
        if (diag) { c_re = NaN; c_im = NaN; }
        if (measure == SC_M_COHERENCY) return make_double2(c_re, c_im);
        if (measure == SC_M_COHERENCE_MAGNITUDE) {
            const double mag = c_re * c_re + c_im * c_im;
            return make_double2((diag ? NaN : measure_clip01(mag)), 0.0);
        }
        return make_double2((diag ? NaN : atan2(c_im, c_re)), 0.0);
    }
    case SC_M_IMAGINARY_COHERENCE: {
        const double den = measure_floor_eps(sqrt(p_i * p_j));
        return make_double2(measure_clip01(fabs(s_im / den)), 0.0);
    }
    case SC_M_PLV:
        return make_double2((sqrt(v.u_re * v.u_re + v.u_im * v.u_im) * rn), 0.0);
    case SC_M_PLV_COMPLEX:
        return make_double2((v.u_re * rn), (v.u_im * rn));
    case SC_M_PPC:
        return make_double2(((v.u_re * v.u_re + v.u_im * v.u_im - n) / (n * n - n)), 0.0);
    case SC_M_PLI:
    case SC_M_DEBIASED_PLI2: {
        const double pli = (diag ? 0.0 : v.sg) * rn;
        return make_double2((measure == SC_M_PLI ? pli : (n * pli * pli - 1.0) / (n - 1.0)), 0.0);
    }
    case SC_M_WPLI: {
        double w = diag ? 0.0 : v.sa * rn;
        if (w < SC_EPS64) w = 1.0;
        return make_double2((s_im * measure_rcp(w)), 0.0);
    }
    case SC_M_DEBIASED_WPLI2: {
        const double si = s_im * n;
        const double sa = diag ? 0.0 : v.sa, sq = diag ? 0.0 : v.sq;
        double wgt = sa * sa - sq;
        if (wgt == 0.0 || n <= 1.0) wgt = NaN;
        return make_double2(((si * si - sq) / wgt), 0.0);
    }
    default:
        return make_double2(0.f, 0.0);
    }
}
