"""CPU checks of the NumPy reference of conditional spectral Granger prediction (tests/conditional_granger_ref.py) on exact VAR
spectra: the explicit Ding et al. normalisation equals the closed form the device computes, the mean over all bins equals
Geweke's time-domain value, conditioning removes the indirect edge of a chain, and two signals give the pairwise measure."""
import numpy as np

import conditional_granger_ref as cref
from oracle import spectral_oracle as so


def chain_var():
    """x -> y -> z (no direct x -> z), correlated innovations, VAR(2)."""
    A = np.zeros((2, 3, 3))
    A[0, 0, 0], A[0, 1, 0], A[0, 1, 1], A[0, 2, 1], A[0, 2, 2], A[1, 2, 2] = 0.5, 0.6, 0.3, 0.6, 0.2, -0.3
    sigma = np.array([[1.0, 0.2, 0.0], [0.2, 1.0, 0.1], [0.0, 0.1, 1.0]])
    return A, sigma


def random_var(C, seed, scale=0.35):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((1, C, C)) * (rng.random((1, C, C)) < 0.4)
    A *= scale / max(np.abs(np.linalg.eigvals(A[0])).max(), 1e-3)
    L = np.eye(C) + 0.2 * np.tril(rng.standard_normal((C, C)), -1)
    return A, L @ L.T


def test_ding_construction_equals_closed_form():
    for A, sigma, N in (chain_var() + (64,), random_var(4, 1) + (32,), random_var(5, 2) + (16,)):
        S = cref.var_spectrum(A, sigma, N)
        ding, closed = cref.conditional_granger_ding(S), cref.conditional_granger_closed(S)
        assert np.array_equal(np.isnan(ding), np.isnan(closed))
        np.testing.assert_allclose(closed, ding, rtol=1e-10, atol=1e-12, equal_nan=True)


def test_integral_identity():
    for A, sigma, N in (chain_var() + (64,), random_var(4, 3) + (64,)):
        S = cref.var_spectrum(A, sigma, N)
        F = cref.conditional_granger_closed(S)
        td = cref.time_domain_conditional(S)
        coupled = td > 1e-3
        assert coupled.sum() >= 2
        mean = cref.two_sided_mean(np.nan_to_num(F), N)
        np.testing.assert_allclose(mean[coupled], td[coupled], rtol=0, atol=1e-8)


def test_chain_indirect_edge_removed():
    A, sigma = chain_var()
    S = cref.var_spectrum(A, sigma, 64)
    cond = cref.conditional_granger_closed(S)
    pair = so.pairwise_spectral_granger_prediction(cref.coefficients_for(S), "tapers")[0, 0]
    assert np.nanmax(np.nan_to_num(cond[:, 2, 0])) < 1e-6          # x -> z given y: nothing
    assert np.nanmax(pair[:, 2, 0]) > 0.1                           # pairwise x -> z: the false edge
    assert np.nanmin(cond[:, 1, 0]) > 0.01 and np.nanmin(cond[:, 2, 1]) > 0.01


def test_two_signals_equal_pairwise():
    A, sigma = chain_var()
    S = cref.var_spectrum(A, sigma, 64)[:, :2, :2]
    cond = cref.conditional_granger_closed(S)
    pair = so.pairwise_spectral_granger_prediction(cref.coefficients_for(S), "tapers")[0, 0]
    assert np.array_equal(np.isnan(cond), np.isnan(pair))
    np.testing.assert_allclose(cond, pair, rtol=0, atol=1e-7, equal_nan=True)


def test_coefficients_reproduce_the_spectrum():
    A, sigma = random_var(5, 4)
    S = cref.var_spectrum(A, sigma, 16)
    coef = cref.coefficients_for(S)
    np.testing.assert_allclose(so.expectation_csm_gemm(coef, "tapers")[0, 0], S, rtol=1e-12, atol=1e-13)
