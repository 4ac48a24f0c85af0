"""The yardstick of the float64 stage-B tests (tests/stage_b_sums_ref.py) against the NumPy oracle, its bounds against a float64
restatement of the device arithmetic summed in another order, and three planted errors against the bounds -- no GPU."""
import numpy as np
import pytest

from oracle import spectral_oracle as so
import stage_b_sums_ref as ref

SHAPES = [(5, 70), (47, 70), (65, 70), (129, 70), (256, 70)]        # (signals, observations per bin)


def _case(C, n_obs, F=1):
    coef = ref.coefficients(F, n_obs, C, seed=1000 * C + n_obs)
    return coef, ref.stage_b_sums(coef)


@pytest.fixture(scope="module")
def case65():
    coef, sums = _case(65, 70, F=2)
    return coef, sums, ref.restatement_f64(coef)


def test_reference_sums_against_the_oracle():
    """A small multitaper case, expectation over trials and tapers: every window is one group of R K observations.  S / n against
    so.expectation_csm_gemm within the bound of a float64 sum (the oracle's own rounding), and the oracle's wPLI, PLV and PLI
    against the same measures built from the longdouble sums: 1e-13 absolute on values of at most 1 (the ratio Im S / sum |Im s|
    of float64 sums of ~20 terms)."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((160, 4, 6))
    x[:, :, 1:] += 0.5 * x[:, :, :-1]
    coef, _ = so.multitaper_fft(x, fs=200.0, NW=3, n_time_samples_per_window=64, n_time_samples_per_step=48)
    W, R, K, N, C = coef.shape
    n = R * K
    csm = so.expectation_csm_gemm(coef)                                      # (W, N, C, C)
    wpli, plv, pli = so.weighted_phase_lag_index(coef), so.phase_locking_value(coef), so.phase_lag_index(coef)
    nn = N // 2 + 1
    diag = np.eye(C, dtype=bool)
    for w in range(W):
        sums = ref.stage_b_sums(np.ascontiguousarray(np.moveaxis(coef[w], 2, 0).reshape(N, n, C)))
        assert sums["near_zero"] == 2 * n * C * (C - 1) // 2            # the DC and Nyquist bins are real: d = 0 exactly there
        b = ref.bounds(sums)
        assert np.all(np.abs(csm[w].real * n - sums["S_re"]) <= b["S_re"])
        assert np.all(np.abs(csm[w].imag * n - sums["S_im"]) <= b["S_im"])
        A = np.where(diag, 0, sums["A"][:nn])
        my_wpli = np.where(diag, 0, sums["S_im"][:nn]) / np.where(A / n < so.EPS, n, A)
        assert np.abs(my_wpli - wpli[w]).max() <= 1e-13
        assert np.abs(np.hypot(sums["U_re"][:nn], sums["U_im"][:nn]) / n - plv[w]).max() <= 1e-13
        assert np.array_equal(np.where(diag, 0, sums["G"][:nn]).astype(np.float64) / n, pli[w])


@pytest.mark.parametrize("C,n_obs", SHAPES)
def test_float64_restatement_stays_inside_every_bound(C, n_obs):
    coef, sums = _case(C, n_obs)
    assert sums["near_zero"] == 0
    worst = ref.worst_ratios(ref.restatement_f64(coef), ref.PLANES, sums)
    print(f"\n  {C:3d} signals x {n_obs} observations, float64 restatement err / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for name, r in worst.items():
        assert r <= 1.0, (name, r)
    assert worst["G"] == 0.0


def test_a_dropped_observation_exceeds_the_bounds(case65):
    coef, sums, _ = case65
    worst = ref.worst_ratios(ref.restatement_f64(coef[:, :-1]), ref.PLANES, sums)
    for name in ("S_re", "S_im", "A", "Q", "U_re", "U_im"):
        assert worst[name] > 1e6, (name, worst[name])
    assert worst["G"] == np.inf


def test_a_tile_from_its_transposed_position_exceeds_the_bounds(case65):
    """Tile (1, 3) of the record filled from the block (3, 1) of the full matrix: transposed inside the tile, Im s negated."""
    _, sums, rec = case65
    bad = rec.copy()
    bad[:, :, 16:32, 48:64] = rec[:, :, 48:64, 16:32]
    assert all(r <= 1.0 for r in ref.worst_ratios(rec, ref.PLANES, sums).values())
    worst = ref.worst_ratios(bad, ref.PLANES, sums)
    for name in ref.PLANES:
        assert worst[name] > 1e6, (name, worst[name])


def test_the_mirror_half_of_a_diagonal_tile_is_not_compared(case65):
    """The checks read the UPPER triangle i <= j only -- what the consumers of a record read; the lower half of a diagonal 16 x 16
    tile is filled by the kernels but mirrored from the upper half by every reader.  A negated sign sum at (i, j) = (22, 19) of the
    diagonal tile 1 therefore changes nothing; the same at (19, 22) does."""
    _, sums, rec = case65
    g = ref.PLANES.index("G")
    assert rec[0, g, 22, 19] != 0
    bad = rec.copy()
    bad[0, g, 22, 19] = -bad[0, g, 22, 19]
    assert ref.worst_ratios(bad, ref.PLANES, sums) == ref.worst_ratios(rec, ref.PLANES, sums)
    bad = rec.copy()
    bad[0, g, 19, 22] = -bad[0, g, 19, 22]
    assert ref.worst_ratios(bad, ref.PLANES, sums)["G"] == np.inf


def test_grouped_observations_follow_the_record_order():
    F, W, R, K, C = 2, 3, 2, 5, 4
    coef5 = np.arange(F * W * R * K * C, dtype=np.float64).reshape(F, W, R, K, C).astype(np.complex128)
    x, n = ref.grouped_observations(coef5, so.EXPECTATION_AXES["time_tapers"])        # trials kept
    assert n == W * K and x.shape == (R * F, n, C)
    for r in range(R):
        for f in range(F):
            assert sorted(x[r * F + f, :, 0].real) == sorted(coef5[f, :, r, :, 0].real.ravel())
