"""NumPy float64 reference of Connectivity.seed_jackknife: the delete-one jackknife of a few signals (seeds) against a list of
signals (targets) for the six pair measures of Connectivity.jackknife.

The yardstick is the all-pairs references indexed at the seeds and targets: ``jackknife`` = jackknife_ref.jackknife (coherence
magnitude on the Fisher scale, signed imaginary coherence) and phase_lag_jackknife_ref.jackknife (the phase-lag family) at
[..., seeds, :][..., targets].  Entry (s, t) is that of the cross-spectrum x_seed conj(x_target): the antisymmetric measures carry
its sign, and where a seed is its own target the entry is the all-pairs diagonal, NaN in all three outputs.

``jackknife_brute_force`` is an independent form that must agree with it: the unit's rows are deleted from the coefficient array,
and every measure is recomputed from scratch from the products of the seed and target columns only -- no all-pairs array, no
subtraction of unit sums.
"""
import numpy as np

import jackknife_ref as jref
import phase_lag_jackknife_ref as pref

FIRST = ("coherence_magnitude", "imaginary_coherence")
MEASURES = FIRST + pref.MEASURES
ANTISYMMETRIC = ("imaginary_coherence",) + pref.ANTISYMMETRIC
OUTPUTS = ("estimate", "bias_corrected", "standard_error")


def from_full(full, seeds, targets):
    """[..., C, C] -> [..., n_seeds, n_targets]"""
    return np.asarray(full)[..., np.asarray(seeds), :][..., np.asarray(targets)]


def jackknife(coefficients, expectation_type, seeds, targets=None, measures=MEASURES, over="trials"):
    """{measure: {estimate, bias_corrected, standard_error}} [kept..., n_freq, n_seeds, n_targets], from the all-pairs references."""
    targets = np.arange(np.shape(coefficients)[-1]) if targets is None else targets
    full = {}
    first, phase = [m for m in measures if m in FIRST], [m for m in measures if m in pref.MEASURES]
    if first:
        full.update(jref.jackknife(coefficients, expectation_type, first, over))
    if phase:
        full.update(pref.jackknife(coefficients, expectation_type, phase, over))
    return {m: {o: from_full(full[m][o], seeds, targets) for o in OUTPUTS} for m in measures}


def _theta(xs, xt, own, measure):
    """The statistic of one set of observations.  xs [..., units, g, n_freq, n_seeds], xt [..., units, g, n_freq, n_targets]."""
    s = xs[..., :, None] * np.conj(xt[..., None, :])                   # [..., units, g, n_freq, n_seeds, n_targets]
    axes = (-5, -4)
    m = s.shape[-5] * s.shape[-4]
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure in FIRST:
            ps, pt = (np.abs(xs) ** 2).sum((-4, -3)), (np.abs(xt) ** 2).sum((-4, -3))
            norm = np.sqrt(ps[..., :, None] * pt[..., None, :])
            S = s.sum(axes)
            out = np.arctanh(np.abs(S) / norm) if measure == "coherence_magnitude" else S.imag / norm
        else:
            im = s.imag
            if measure == "phase_lag_index":
                out = np.sign(im).sum(axes) / m
            elif measure == "debiased_squared_phase_lag_index":
                out = (m * (np.sign(im).sum(axes) / m) ** 2 - 1.0) / (m - 1.0)
            elif measure == "weighted_phase_lag_index":
                w = np.abs(im).sum(axes) / m
                out = (im.sum(axes) / m) / np.where(w < pref.EPS, 1.0, w)
            elif measure == "debiased_squared_weighted_phase_lag_index":
                q = (im * im).sum(axes)
                den = np.abs(im).sum(axes) ** 2 - q
                out = (im.sum(axes) ** 2 - q) / np.where(den == 0, np.nan, den)
            else:
                raise ValueError(measure)
    out = np.array(out, dtype=np.float64)
    out[..., own] = np.nan
    return out


def jackknife_brute_force(coefficients, expectation_type, seeds, targets=None, measures=MEASURES, over="trials"):
    """The unit is deleted from the coefficient array and every measure recomputed for the seed-target entries only."""
    x = jref.units(coefficients, expectation_type, over)
    seeds = np.asarray(seeds)
    targets = np.arange(x.shape[-1]) if targets is None else np.asarray(targets)
    own = seeds[:, None] == targets[None, :]
    n = x.shape[-4]
    out = {}
    for measure in measures:
        theta = _theta(x[..., seeds], x[..., targets], own, measure)
        d = np.empty((n,) + theta.shape)
        for u in range(n):
            rest = np.delete(x, u, axis=-4)
            d[u] = _theta(rest[..., seeds], rest[..., targets], own, measure) - theta
        mean = d.mean(axis=0)
        out[measure] = dict(estimate=theta, bias_corrected=theta - (n - 1) * mean,
                            standard_error=np.sqrt((n - 1) / n * ((d - mean) ** 2).sum(axis=0)))
    return out
