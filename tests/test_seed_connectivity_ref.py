"""tests/seed_connectivity_ref.py -- the float64 NumPy restatement of the seed record and the seed epilogue (csrc/sc_seed.hip) -- held
to the oracle's ten all-pairs functions, indexed [..., seeds, :][..., targets], at 1e-12.  No device."""
import numpy as np
import pytest

import seed_connectivity_ref as sref
from oracle import spectral_oracle as so

TOL = 1e-12


def coefficients(shape, seed, real_bins=True):
    rng = np.random.default_rng(seed)
    coef = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if real_bins:                       # a real series: the zero and Nyquist bins are real (Im s = 0, sign 0, debiased wPLI NaN)
        coef[:, :, :, 0] = coef[:, :, :, 0].real
        coef[:, :, :, shape[3] // 2] = coef[:, :, :, shape[3] // 2].real
    return coef


def assert_equal_to_oracle(coef, seeds, targets, expectation_type, measures=sref.MEASURES):
    got = sref.seed_connectivity(coef, seeds, targets, measures, expectation_type=expectation_type)
    assert tuple(got) == tuple(measures)
    t = np.arange(coef.shape[-1]) if targets is None else targets
    for name in measures:
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = sref.from_full(getattr(so, name)(coef, expectation_type), seeds, t)
        assert got[name].shape == ref.shape, name
        assert np.array_equal(np.isnan(got[name]), np.isnan(ref)), f"{name}: NaN pattern"
        ok = ~np.isnan(ref) & ~np.isinf(ref)
        assert np.array_equal(got[name][np.isinf(ref)], ref[np.isinf(ref)]), f"{name}: infinities"
        if not ok.any():
            continue
        assert np.abs(got[name][ok] - ref[ok]).max() <= TOL * max(1.0, np.abs(ref[ok]).max()), name


@pytest.mark.parametrize("expectation_type", list(sref.EXPECTATION_AXES))
def test_every_expectation_type(expectation_type):
    coef = coefficients((3, 4, 2, 8, 7), 1)
    assert_equal_to_oracle(coef, [5, 0], None, expectation_type)


def test_seeds_among_permuted_and_subset_targets():
    coef = coefficients((2, 5, 3, 16, 9), 2)
    assert_equal_to_oracle(coef, [7, 2, 4], [8, 2, 0, 7, 5], "trials_tapers")
    assert_equal_to_oracle(coef, [3], [3], "time_trials_tapers")


def test_degenerate_cases():
    # one observation: the debiased measures (NaN, -inf where sign Im s = 0).  Not the pairwise phase consistency: (|u|^2 - 1) / 0
    # of a unit phasor u is +-inf or NaN by the rounding of |u|^2, in the reference too.
    coef = coefficients((1, 1, 1, 8, 5), 3)
    assert_equal_to_oracle(coef, [1, 4], None, "trials_tapers", [m for m in sref.MEASURES if m != "pairwise_phase_consistency"])
    coef = coefficients((1, 6, 2, 8, 5), 4)
    coef[..., 2] = 0.0                                       # a channel without power: eps floors, 0 / 0 unit phasors
    assert_equal_to_oracle(coef, [2, 0], None, "trials_tapers")
    coef = coefficients((1, 6, 2, 8, 5), 5)
    coef[0, 3, 1, 2, 4] = 0.0                                # one coefficient of modulus 0
    assert_equal_to_oracle(coef, [4, 1], [0, 4, 3], "trials_tapers")


def test_sign_follows_seed_conj_target():
    coef = coefficients((1, 8, 2, 8, 4), 6, real_bins=False)
    a = sref.seed_connectivity(coef, [0], [1], ("weighted_phase_lag_index", "phase_lag_index", "coherence_phase"))
    b = sref.seed_connectivity(coef, [1], [0], ("weighted_phase_lag_index", "phase_lag_index", "coherence_phase"))
    for name in a:
        np.testing.assert_allclose(a[name], -b[name], rtol=0, atol=1e-15)
