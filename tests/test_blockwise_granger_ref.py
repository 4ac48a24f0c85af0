"""CPU checks of the NumPy reference of blockwise spectral Granger prediction (tests/blockwise_granger_ref.py) on exact VAR
spectra: Geweke's explicit construction, the reference form and the null-space form the device computes agree; singleton blocks
give the pairwise measure; the measure is invariant under invertible mixing inside each block; a one-way VAR gives zero in the
other direction; the mean over all bins equals Geweke's time-domain value."""
import numpy as np

import blockwise_granger_ref as bref
import conditional_granger_ref as cref
from oracle import spectral_oracle as so


def random_var(C, seed, scale=0.35):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((1, C, C)) * (rng.random((1, C, C)) < 0.5)
    A *= scale / max(np.abs(np.linalg.eigvals(A[0])).max(), 1e-3)
    L = np.eye(C) + 0.2 * np.tril(rng.standard_normal((C, C)), -1)
    return A, L @ L.T


def one_way_var():
    """Block b = signals (2, 3, 4) drives block a = (0, 1); nothing goes from a to b.  VAR(1) with a block lower-triangular
    coefficient matrix whose diagonal blocks are stable: det H~_aa(z) = det(I - A_aa z)^-1 has no zeros in the unit disc
    (Geweke's condition for the integral identity), and the innovations are correlated across the blocks."""
    A = np.zeros((1, 5, 5))
    A[0, :2, :2] = [[0.5, 0.1], [-0.2, 0.3]]
    A[0, 2:, 2:] = [[0.4, 0.2, 0.0], [0.0, -0.3, 0.1], [0.1, 0.0, 0.2]]
    A[0, :2, 2:] = [[0.5, 0.0, -0.3], [0.2, 0.4, 0.0]]
    sigma = np.eye(5)
    sigma[0, 2] = sigma[2, 0] = 0.3
    sigma[1, 4] = sigma[4, 1] = -0.2
    return A, sigma


def test_three_forms_agree():
    """At a Wilson tolerance of 1e-14 (enough bins that the factor reproduces the spectrum: the model and the input S_aa of the
    forms then agree to rounding)."""
    for C, labels, seed, N in ((5, [0, 1, 1, 0, 1], 1, 64), (6, ["x", "y", "x", "z", "y", "y"], 2, 128), (4, [2, 2, 7, 7], 3, 64)):
        A, sigma = random_var(C, seed)
        S = cref.var_spectrum(A, sigma, N)
        ref, labs = bref.blockwise_granger(S, labels, "nullspace", tolerance=1e-14)
        assert list(labs) == sorted(set(labels))
        assert np.isnan(ref[:, range(len(labs)), range(len(labs))]).all()
        assert np.isfinite(ref).sum() > 0.5 * (ref.size - ref.shape[0] * len(labs))
        for form in ("geweke", "reference"):
            other, _ = bref.blockwise_granger(S, labels, form, tolerance=1e-14)
            assert np.array_equal(np.isnan(other), np.isnan(ref)), form
            np.testing.assert_allclose(other, ref, rtol=0, atol=1e-12, equal_nan=True, err_msg=form)


def test_singleton_blocks_equal_pairwise():
    """Separate Wilson iterations (2 x 2 problems in both, stopped at the tolerance 1e-8): agreement to the tolerance."""
    for C, seed in ((3, 4), (5, 5)):
        A, sigma = random_var(C, seed)
        S = cref.var_spectrum(A, sigma, 64)
        bw, _ = bref.blockwise_granger(S, np.arange(C))
        pw = so.pairwise_spectral_granger_prediction(cref.coefficients_for(S), "tapers")[0, 0]
        assert np.array_equal(np.isnan(bw), np.isnan(pw))
        np.testing.assert_allclose(bw, pw, rtol=0, atol=1e-8, equal_nan=True)


def test_invariant_under_mixing_inside_blocks():
    """S -> T S T^H with T = blockdiag(A_a, A_b): Geweke's invariance.  The two spectra go through separate Wilson iterations
    at the tolerance 1e-8, so 1e-6, not rounding."""
    rng = np.random.default_rng(6)
    for C, labels in ((5, np.array([0, 1, 1, 0, 1])), (7, np.array([0, 1, 2, 0, 2, 1, 2]))):
        A, sigma = random_var(C, 10 + C)
        S = cref.var_spectrum(A, sigma, 64)
        T = np.zeros((C, C))
        for lab in np.unique(labels):
            idx = np.flatnonzero(labels == lab)
            T[np.ix_(idx, idx)] = np.eye(len(idx)) + 0.5 * rng.standard_normal((len(idx), len(idx)))
        ref, _ = bref.blockwise_granger(S, labels)
        mixed, _ = bref.blockwise_granger(T @ S @ T.T, labels)
        assert np.array_equal(np.isnan(mixed), np.isnan(ref))
        np.testing.assert_allclose(mixed, ref, rtol=0, atol=1e-6, equal_nan=True)
        # mixing ACROSS blocks is not an invariance: the test above can fail
        T2 = np.eye(C) + 0.5 * rng.standard_normal((C, C))
        assert np.nanmax(np.abs(bref.blockwise_granger(T2 @ S @ T2.T, labels)[0] - ref)) > 1e-3


def test_one_way_var():
    A, sigma = one_way_var()
    N = 64
    S = cref.var_spectrum(A, sigma, N)
    labels = np.array([0, 0, 1, 1, 1])
    F, _ = bref.blockwise_granger(S, labels)
    a_to_b, b_to_a = F[:, 1, 0], F[:, 0, 1]
    assert np.nan_to_num(a_to_b).max() < 1e-8
    assert b_to_a.min() > 0.01
    # Geweke's integral identity (the condition holds: see one_way_var)
    mean = cref.two_sided_mean(np.nan_to_num(F), N)
    td = bref.time_domain_blockwise(S, np.array([0, 1]), np.array([2, 3, 4]))
    np.testing.assert_allclose(mean[0, 1], td, rtol=0, atol=1e-8)
    assert td > 0.05


def test_embedding_leaves_the_measure_unchanged():
    """The construction the GPU tests use for large blocks: independent processes added to the blocks and mixing inside
    every block leave each pair's measure equal to that of the small core."""
    A, sigma = random_var(5, 8)
    core = cref.var_spectrum(A, sigma, 32)
    core_labels = np.array([0, 1, 1, 0, 2])
    S, labels = bref.embed(core, core_labels, [6, 4, 5], seed=9)
    ref, _ = bref.blockwise_granger(core, core_labels)
    got, _ = bref.blockwise_granger(S, labels)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6, equal_nan=True)
