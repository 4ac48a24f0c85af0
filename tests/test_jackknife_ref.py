"""The jackknife yardstick (tests/jackknife_ref.py) against itself and against theory, the host-side interval function and the
argument checks of Connectivity.jackknife -- no GPU."""
import numpy as np
import pytest
import scipy.stats

import jackknife_ref as jref

OUTPUTS = ("estimate", "bias_corrected", "standard_error")
THREE = ("power", "coherence_magnitude", "imaginary_coherence")


def assert_same(a, b, tol, what):
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN patterns differ"
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]) - tol * (1 + np.abs(b[ok]))
    assert err.max() <= 0, f"{what}: worst excess {err.max():.3e}"


@pytest.mark.parametrize("shape,expectation_type,over", [
    ((1, 1000, 7, 3, 4), "trials_tapers", "trials"),
    ((3, 12, 4, 5, 5), "time_trials_tapers", "trials"),
    ((2, 1, 9, 5, 4), "tapers", "observations"),
    ((2, 6, 3, 5, 3), "trials_tapers", "observations"),
])
def test_subtract_form_equals_brute_force(shape, expectation_type, over):
    """(a) S - G_u against deleting the unit and recomputing: 1e-10 relative + absolute on all three outputs."""
    coef = jref.mixed_noise(*shape, seed=3)
    a = jref.jackknife(coef, expectation_type, THREE, over)
    b = jref.jackknife_brute_force(coef, expectation_type, THREE, over)
    W, R, K, F, C = shape
    kept = {"trials_tapers": (W,), "time_trials_tapers": (), "tapers": (W, R)}[expectation_type]
    for m in THREE:
        assert a[m]["estimate"].shape == kept + (F, C) + ((C,) if m != "power" else ())
        for o in OUTPUTS:
            assert_same(a[m][o], b[m][o], 1e-10, f"{m} {o}")
    off = ~np.eye(C, dtype=bool)
    assert np.isnan(a["coherence_magnitude"]["estimate"][..., ~off]).all()
    ic = a["imaginary_coherence"]["estimate"]
    assert np.allclose(ic[..., off], -np.swapaxes(ic, -1, -2)[..., off])


def test_linear_statistic_identity():
    """(b) For the untransformed S_ii / n_obs the jackknife standard error is std(per-unit power, ddof=1) / sqrt(n) exactly, and
    the bias correction is nothing."""
    W, R, K, F, C = 2, 30, 5, 6, 4
    coef = jref.mixed_noise(W, R, K, F, C, seed=5)
    r = jref.jackknife(coef, "trials_tapers", ("linear_power",))["linear_power"]
    per_unit = (np.abs(coef[:, :, :, :F]) ** 2).mean(axis=2)              # (W, R, F, C): a trial's own power
    want = per_unit.std(axis=1, ddof=1) / np.sqrt(R)
    np.testing.assert_allclose(r["standard_error"], want, rtol=1e-12)
    np.testing.assert_allclose(r["bias_corrected"], r["estimate"], rtol=1e-12)
    np.testing.assert_allclose(r["estimate"], per_unit.mean(axis=1), rtol=1e-12)


def test_fisher_z_calibration():
    """(c) Mixed complex Gaussian noise: the mean Fisher-z standard error over the off-diagonal entries is within 5 % of the
    asymptotic 1 / sqrt(2 R K - 2)."""
    W, R, K, F, C = 2, 40, 5, 17, 6
    coef = jref.mixed_noise(W, R, K, F, C, seed=0)
    se = jref.jackknife(coef, "trials_tapers", ("coherence_magnitude",))["coherence_magnitude"]["standard_error"]
    off = ~np.eye(C, dtype=bool)
    mean, want = se[..., off].mean(), 1.0 / np.sqrt(2 * R * K - 2)
    print(f"mean Fisher-z standard error {mean:.5f}, asymptotic {want:.5f} ({100 * (mean / want - 1):+.1f} %)")
    assert abs(mean / want - 1) <= 0.05


def test_confidence_intervals():
    """(d) statistics.jackknife_confidence_intervals: the hand formula, contains the back-transformed estimate, widens with ci."""
    from spectral_connectivity_amd.statistics import JackknifeResult, jackknife_confidence_intervals
    # strongly mixed channels: a coherence near 0 has a Fisher-z bias of the order of its standard error, and the bias-corrected
    # interval then need not contain the uncorrected estimate; here the correction is under 0.13 of the half width
    coef = jref.mixed_noise(1, 30, 3, 5, 4, seed=7, mix=1.0)
    ref = jref.jackknife(coef, "trials_tapers", THREE)
    for name, transform, back in (("power", "log", np.exp), ("coherence_magnitude", "fisher_z", np.tanh),
                                  ("imaginary_coherence", "identity", lambda v: v)):
        r = JackknifeResult(ref[name]["estimate"], ref[name]["bias_corrected"], ref[name]["standard_error"], transform, 30, "trials")
        lo, hi = jackknife_confidence_intervals(r, ci=0.95)
        t = scipy.stats.t.ppf(0.975, 29)
        np.testing.assert_allclose(lo, back(r.bias_corrected - t * r.standard_error), rtol=1e-13, equal_nan=True)
        np.testing.assert_allclose(hi, back(r.bias_corrected + t * r.standard_error), rtol=1e-13, equal_nan=True)
        ok = ~np.isnan(lo)
        assert ok.any() and np.all(lo[ok] < hi[ok])
        centre = back(r.bias_corrected)
        assert np.all(lo[ok] <= centre[ok]) and np.all(centre[ok] <= hi[ok])
        est = back(r.estimate)
        assert np.all(lo[ok] <= est[ok]) and np.all(est[ok] <= hi[ok])
        lo3, hi3 = jackknife_confidence_intervals(r, ci=0.999)
        assert np.all(lo3[ok] < lo[ok]) and np.all(hi3[ok] > hi[ok])
    with pytest.raises(ValueError, match="between 0 and 1"):
        jackknife_confidence_intervals(r, ci=1.0)


def test_request_is_checked_before_the_device():
    """(e) Every ValueError of Connectivity.jackknife comes from the host: this process has no GPU."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)

    def conn(shape, expectation_type):
        return sc.Connectivity(rng.standard_normal(shape) + 1j * rng.standard_normal(shape), expectation_type=expectation_type)

    c = conn((2, 4, 3, 8, 3), "trials_tapers")
    with pytest.raises(ValueError, match="unknown measure 'coherence'.*'power', 'coherence_magnitude', 'imaginary_coherence'"):
        c.jackknife(("coherence",))
    with pytest.raises(ValueError, match="measures is empty.*'power'"):
        c.jackknife(())
    with pytest.raises(ValueError, match="over must be 'trials' or 'observations'"):
        c.jackknife(over="tapers")
    with pytest.raises(ValueError, match="averages over trials.*'trials_tapers'.*got 'tapers'"):
        conn((2, 4, 3, 8, 3), "tapers").jackknife()
    with pytest.raises(ValueError, match="n_trials >= 2"):
        conn((2, 1, 3, 8, 3), "trials_tapers").jackknife()
    with pytest.raises(ValueError, match="n_observations >= 2"):
        conn((2, 4, 1, 8, 3), "tapers").jackknife(over="observations")
