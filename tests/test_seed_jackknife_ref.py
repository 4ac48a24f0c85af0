"""The NumPy reference of Connectivity.seed_jackknife (tests/seed_jackknife_ref.py) against itself: the all-pairs references indexed
at the seeds and targets agree with the brute-force form that deletes a unit's rows and recomputes the seed-target entries only,
and the yardstick has the sign and diagonal rules of the method's contract.  CPU only."""
import numpy as np
import pytest

import jackknife_ref as jref
import phase_lag_jackknife_ref as pref
import seed_jackknife_ref as sjref

# (W, R, K, F, C, expectation_type, over, seeds, targets)
CASES = [
    (2, 2, 3, 5, 2, "trials_tapers", "trials", [1], None),
    (1, 3, 4, 5, 3, "trials_tapers", "trials", [2, 0], None),
    (2, 6, 2, 4, 7, "time_trials_tapers", "trials", [6, 5], [0, 1, 2, 3, 4]),
    (1, 5, 2, 4, 6, "trials_tapers", "observations", [3], [5, 0, 3, 1]),
    (3, 1, 4, 4, 5, "tapers", "observations", [0, 4, 2], [4, 3, 2, 1, 0]),
    (2, 4, 1, 4, 5, "trials", "trials", [1, 3], None),
]


def close(a, b, what, tol=1e-9):
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN patterns differ"
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]) / (1 + np.abs(b[ok]))
    assert err.size == 0 or err.max() <= tol, f"{what}: {err.max():.3e}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c[:7]))
@pytest.mark.parametrize("maker", ["lagged_noise", "margin_phases"])
def test_indexed_all_pairs_agrees_with_brute_force(case, maker):
    W, R, K, F, C, expectation_type, over, seeds, targets = case
    coef = getattr(pref, maker)(W, R, K, F, C, seed=C + R)
    a = sjref.jackknife(coef, expectation_type, seeds, targets, over=over)
    b = sjref.jackknife_brute_force(coef, expectation_type, seeds, targets, over=over)
    n_targets = C if targets is None else len(targets)
    for m in sjref.MEASURES:
        for o in sjref.OUTPUTS:
            assert a[m][o].shape[-3:] == (F, len(seeds), n_targets), (m, o)
            # (a standard error is the root of a sum of squares: a reference value of exactly 0 and one of 1e-17 are both right)
            close(a[m][o], b[m][o], f"{m} {o}", 1e-9 if o != "standard_error" else 1e-8)
    # off the seed-is-target entries the yardstick is finite on these inputs
    own = np.asarray(seeds)[:, None] == (np.arange(C) if targets is None else np.asarray(targets))[None, :]
    for m in sjref.MEASURES:
        if (m, over, R * K * W) == ("coherence_magnitude", "observations", 2):
            continue
        for o in sjref.OUTPUTS:
            assert np.isfinite(a[m][o][..., ~own]).all(), (m, o)
            assert np.isnan(a[m][o][..., own]).all(), (m, o)


def test_a_seed_above_its_target_has_the_negated_antisymmetric_entries():
    coef = pref.lagged_noise(2, 5, 3, 5, 6, seed=3)
    up = sjref.jackknife(coef, "trials_tapers", [1], [4])
    down = sjref.jackknife(coef, "trials_tapers", [4], [1])
    for m in sjref.MEASURES:
        sign = -1.0 if m in sjref.ANTISYMMETRIC else 1.0
        assert np.abs(up[m]["estimate"]).max() > 0
        # theta and sum d change sign (estimate, bias_corrected), sum d^2 does not (standard_error)
        assert np.array_equal(down[m]["estimate"], sign * up[m]["estimate"]), m
        assert np.allclose(down[m]["bias_corrected"], sign * up[m]["bias_corrected"], rtol=1e-12, atol=0), m
        assert np.allclose(down[m]["standard_error"], up[m]["standard_error"], rtol=1e-12, atol=0), m
    for form in (sjref.jackknife, sjref.jackknife_brute_force):
        both = form(coef, "trials_tapers", [4, 1], [1, 4], measures=("weighted_phase_lag_index",))["weighted_phase_lag_index"]
        assert np.allclose(both["estimate"][..., 0, 0], -both["estimate"][..., 1, 1], rtol=1e-12, atol=0)
        assert (np.abs(both["estimate"][..., 0, 0]) > 1e-3).any()


def test_a_seed_that_is_its_own_target_is_nan_in_all_three_outputs():
    coef = pref.margin_phases(1, 4, 2, 4, 5, seed=8)
    for form in (sjref.jackknife, sjref.jackknife_brute_force):
        got = form(coef, "trials_tapers", [3, 0], [0, 1, 3])
        for m in sjref.MEASURES:
            for o in sjref.OUTPUTS:
                v = got[m][o]
                assert np.isnan(v[..., 0, 2]).all() and np.isnan(v[..., 1, 0]).all(), (m, o)
                rest = np.ones((2, 3), dtype=bool)
                rest[0, 2] = rest[1, 0] = False
                assert np.isfinite(v[..., rest]).all(), (m, o)


def test_the_yardstick_is_the_all_pairs_references_unchanged():
    coef = pref.lagged_noise(1, 4, 3, 5, 4, seed=5)
    got = sjref.jackknife(coef, "trials_tapers", [2], None)
    first = jref.jackknife(coef, "trials_tapers", sjref.FIRST)
    phase = pref.jackknife(coef, "trials_tapers")
    for m in sjref.MEASURES:
        full = (first if m in sjref.FIRST else phase)[m]
        for o in sjref.OUTPUTS:
            assert np.array_equal(got[m][o], full[o][..., 2:3, :], equal_nan=True), (m, o)


def gpu_cases():
    import test_gpu_seed_jackknife as gpu
    return [(c, "lagged_noise") for c in gpu.PARITY_CASES] + [(c, "margin_phases") for c in gpu.MARGIN_CASES]


@pytest.mark.parametrize("case,maker", gpu_cases(), ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v[:7]) + f"-{len(v[7])}")
def test_the_yardstick_of_every_device_case_is_finite_off_its_nan_entries(case, maker):
    """The cases of tests/test_gpu_seed_jackknife.py: all three outputs of all six measures are finite, except where a seed is its
    own target."""
    import test_gpu_seed_jackknife as gpu
    _, ref = gpu.inputs_and_reference(case, maker)
    targets = np.arange(case[4]) if case[8] is None else np.asarray(case[8])
    own = np.asarray(case[7])[:, None] == targets[None, :]
    for m in sjref.MEASURES:
        for o in sjref.OUTPUTS:
            assert np.isnan(ref[m][o][..., own]).all() and np.isfinite(ref[m][o][..., ~own]).all(), (m, o)
