"""The NumPy float64 reference of the total, instantaneous and lagged linear dependence (tests/linear_dependence_ref.py) against
itself: its two forms that share no step, the closed forms of single signals, and the properties the measures are defined by."""
import numpy as np
import pytest

import linear_dependence_ref as lref

SIZES = [(1, 1), (1, 16), (8, 8), (16, 17), (32, 32), (63, 65), (64, 64), (1, 127)]


def case(sizes):
    """(one-sided spectra [17, C, C], permuted labels) of a size pair -- the spectra and labels of the GPU test."""
    na, nb = sizes
    C = na + nb
    S = lref.var_spectrum(C, C)
    labels = np.r_[np.zeros(na, int), np.ones(nb, int)][np.random.default_rng(C).permutation(C)]
    return S[:S.shape[0] // 2 + 1], labels


@pytest.mark.parametrize("sizes", SIZES)
def test_two_forms_agree(sizes):
    S, labels = case(sizes)
    a = lref.dependence(S, labels, form="logdet")
    b = lref.dependence(S, labels, form="canonical")
    for x, y, what in zip(a[:3], b[:3], ("total", "instantaneous", "lagged")):
        err = np.abs(x[:, 0, 1] - y[:, 0, 1]).max()
        print(f"{sizes} {what}: forms differ by {err:.2e}")
        assert err <= 1e-10, (sizes, what, err)
        assert np.array_equal(x[:, 0, 1], x[:, 1, 0]) and np.isnan(x[:, 0, 0]).all()
    assert np.all(a[0][:, 0, 1] > 0) and np.all(a[2][:, 0, 1] >= -1e-12)


def test_single_signals_equal_the_closed_forms():
    S = lref.var_spectrum(7, 3)[:17]
    total, inst, lagged, labels = lref.dependence(S)
    assert list(labels) == list(range(7)) and total.shape == (17, 7, 7)
    ct, ci, cl, rho2 = lref.pairwise_closed(S)
    off = ~np.eye(7, dtype=bool)
    for got, want in ((total, ct), (inst, ci), (lagged, cl)):
        np.testing.assert_allclose(got[:, off], want[:, off], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(-np.expm1(-lagged[:, off]), rho2[:, off], rtol=1e-10, atol=1e-12)
    c = lref.coherency(S, 0, 1)
    np.testing.assert_allclose(rho2[:, 0, 1], c.imag ** 2 / (1 - c.real ** 2), rtol=1e-13)
    assert rho2[1:-1][:, off].max() > 0.01


@pytest.mark.parametrize("form", ["logdet", "canonical"])
def test_total_is_instantaneous_plus_lagged(form):
    S, labels = case((8, 8))
    total, inst, lagged, _ = lref.dependence(S, labels, form=form)
    np.testing.assert_allclose(total[:, 0, 1], inst[:, 0, 1] + lagged[:, 0, 1], rtol=1e-13, atol=1e-14)


def test_lagged_is_zero_for_a_real_spectrum():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((5, 12, 40))
    S = X @ np.swapaxes(X, -1, -2) / 40 + 0j
    labels = np.array([0, 1, 2] * 4)
    for form in ("logdet", "canonical"):
        total, inst, lagged, _ = lref.dependence(S, labels, form=form)
        off = ~np.eye(3, dtype=bool)
        assert np.abs(lagged[:, off]).max() <= 1e-13 and total[:, off].min() > 0.01
    assert np.all(lref.pairwise_closed(S)[2][:, ~np.eye(12, dtype=bool)] == 0.0)


def _mix(C, labels, rng, complex_):
    T = np.zeros((C, C), dtype=complex if complex_ else float)
    for lab in np.unique(labels):
        idx = np.flatnonzero(labels == lab)
        M = np.eye(len(idx)) + 0.5 * rng.standard_normal((len(idx), len(idx))) / np.sqrt(len(idx))
        if complex_:
            M = M + 0.5j * rng.standard_normal((len(idx), len(idx))) / np.sqrt(len(idx))
        T[np.ix_(idx, idx)] = M
    return T


def test_mixing_inside_the_groups():
    """Real invertible mixing inside each group leaves all three unchanged, complex mixing the total."""
    S, labels = case((16, 17))
    rng = np.random.default_rng(6)
    base = lref.dependence(S, labels)
    T = _mix(33, labels, rng, False)
    mixed = lref.dependence(T @ S @ T.T, labels)
    for x, y in zip(base[:3], mixed[:3]):
        np.testing.assert_allclose(y[:, 0, 1], x[:, 0, 1], rtol=1e-9, atol=1e-11)
    T = _mix(33, labels, rng, True)
    mixed = lref.dependence(T @ S @ np.conj(T.T), labels)
    np.testing.assert_allclose(mixed[0][:, 0, 1], base[0][:, 0, 1], rtol=1e-9, atol=1e-11)
    assert np.abs(mixed[1][:, 0, 1] - base[1][:, 0, 1]).max() > 1e-3      # (the instantaneous part is NOT invariant to it)


@pytest.mark.parametrize("sizes", [(1, 16), (8, 8), (16, 17)])
def test_total_from_the_canonical_coherences(sizes):
    S, labels = case(sizes)
    a, b = np.flatnonzero(labels == 0), np.flatnonzero(labels == 1)
    rho2 = lref.canonical_coherences_squared(S, a, b)
    assert rho2.shape[-1] == len(a) and np.all(rho2 < 1) and np.all(rho2 > -1e-12)
    total = lref.dependence(S, labels)[0][:, 0, 1]
    np.testing.assert_allclose(-np.log1p(-rho2).sum(axis=-1), total, rtol=1e-9, atol=1e-11)
