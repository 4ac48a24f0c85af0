"""The phase-lag jackknife yardstick (tests/phase_lag_jackknife_ref.py) against itself, against the project's oracle and against
the properties of its statistics -- no GPU."""
import numpy as np
import pytest

import jackknife_ref as jref
import phase_lag_jackknife_ref as pref
from oracle import spectral_oracle as so

OUTPUTS = ("estimate", "bias_corrected", "standard_error")
ORACLE = {"phase_lag_index": so.phase_lag_index, "weighted_phase_lag_index": so.weighted_phase_lag_index,
          "debiased_squared_phase_lag_index": so.debiased_squared_phase_lag_index,
          "debiased_squared_weighted_phase_lag_index": so.debiased_squared_weighted_phase_lag_index}


def assert_same(a, b, tol, what):
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN patterns differ"
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]) - tol * (1 + np.abs(b[ok]))
    assert err.max() <= 0, f"{what}: worst excess {err.max():.3e}"


# (W, R, K, F, C): g = 1, g = 35, n = 2 and n = 50 among them
@pytest.mark.parametrize("shape,expectation_type,over", [
    ((2, 6, 1, 3, 3), "trials", "trials"),                      # g = 1
    ((5, 3, 7, 3, 3), "time_trials_tapers", "trials"),          # g = 35
    ((2, 2, 3, 5, 4), "trials_tapers", "trials"),               # n = 2
    ((1, 50, 2, 3, 5), "trials_tapers", "trials"),              # n = 50
    ((2, 1, 9, 5, 4), "tapers", "observations"),
    ((2, 6, 3, 5, 3), "trials_tapers", "observations"),
])
def test_subtract_form_equals_brute_force(shape, expectation_type, over):
    coef = pref.lagged_noise(*shape, seed=3)
    a = pref.jackknife(coef, expectation_type, pref.MEASURES, over)
    b = pref.jackknife_brute_force(coef, expectation_type, pref.MEASURES, over)
    x = jref.units(coef, expectation_type, over)
    W, R, K, F, C = shape
    for m in pref.MEASURES:
        assert a[m]["estimate"].shape == x.shape[:-4] + (F, C, C)
        for o in OUTPUTS:
            assert_same(a[m][o], b[m][o], 1e-12, f"{m} {o}")


@pytest.mark.parametrize("expectation_type,over",
                         [(e, "observations") for e in jref.EXPECTATION_AXES] +
                         [(e, "trials") for e, axes in jref.EXPECTATION_AXES.items() if 1 in axes])
def test_estimate_is_the_oracles_measure(expectation_type, over):
    W, R, K, F, C = 3, 4, 2, 5, 4
    coef = pref.lagged_noise(W, R, K, F, C, seed=11)
    got = pref.jackknife(coef, expectation_type, pref.MEASURES, over)
    off = ~np.eye(C, dtype=bool)
    for m in pref.MEASURES:
        want = ORACLE[m](coef, expectation_type)
        est = got[m]["estimate"]
        assert est.shape == want.shape, m
        assert np.isnan(est[..., ~off]).all(), m
        assert_same(est[..., off], want[..., off], 1e-12, f"{m} {expectation_type} {over}")


def test_symmetry():
    C = 5
    coef = pref.lagged_noise(2, 7, 3, 5, C, seed=5)
    got = pref.jackknife(coef, "trials_tapers")
    off = ~np.eye(C, dtype=bool)
    for m in pref.MEASURES:
        sign = -1.0 if m in pref.ANTISYMMETRIC else 1.0
        for o in OUTPUTS:
            v = got[m][o]
            s = 1.0 if o == "standard_error" else sign
            assert np.array_equal(v[..., off], s * np.swapaxes(v, -1, -2)[..., off]), f"{m} {o}"
            assert np.isnan(v[..., ~off]).all(), f"{m} {o}"
    # the true wPLI of the complex mixing is not 0: the yardstick's inputs exercise the signed statistic
    assert np.abs(got["weighted_phase_lag_index"]["estimate"][..., off]).max() > 0.3


def test_bins_without_an_imaginary_part():
    """Im s = 0 in every observation of a bin (the zero and Nyquist bins of a real series): PLI and wPLI are exactly 0 with a
    standard error of exactly 0, the debiased wPLI^2 is NaN (0 / 0 by its definition)."""
    C = 4
    coef = pref.lagged_noise(2, 6, 3, 5, C, seed=7)
    coef[:, :, :, 0] = coef[:, :, :, 0].real
    coef[:, :, :, 4] = coef[:, :, :, 4].real
    got = pref.jackknife(coef, "trials_tapers")
    off = ~np.eye(C, dtype=bool)
    for f in (0, 4):
        for m in pref.ANTISYMMETRIC:
            for o in OUTPUTS:
                assert np.all(got[m][o][:, f][..., off] == 0), f"{m} {o} bin {f}"
        for o in OUTPUTS:
            assert np.isnan(got["debiased_squared_weighted_phase_lag_index"][o][:, f]).all(), f"{o} bin {f}"
    for f in (1, 2, 3):
        assert np.isfinite(got["debiased_squared_weighted_phase_lag_index"]["estimate"][:, f][..., off]).all()


@pytest.mark.parametrize("C", [2, 3, 16, 17, 33])
def test_margin_phases_keep_their_margin(C):
    coef = pref.margin_phases(2, 5, 3, 4, C, seed=C)                  # (asserts its own margin)
    assert coef.shape == (2, 5, 3, 6, C)
    half = coef[:, :, :, :4]
    s = half[..., :, None] * np.conj(half[..., None, :])
    rel = np.abs(s.imag) / np.abs(s)
    off = ~np.eye(C, dtype=bool)
    assert rel[..., off].min() >= np.sin(3 * np.pi / (4 * (C + 1))) * (1 - 1e-12)
    assert np.sin(3 * np.pi / (4 * (C + 1))) >= 0.069
    assert 0.5 <= np.abs(half).min() and np.abs(half).max() <= 2.0
