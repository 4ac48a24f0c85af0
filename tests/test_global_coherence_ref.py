"""The reference of the global-coherence suite (tests/global_coherence_ref.py) checked on the CPU: the ``exact`` family is exact, the
record round-trips, the exact products of ``check`` agree with a plain extended-precision product, and numpy.linalg.eigh passes
``check`` under the committed bars on every case of (a) -- which is what shows the bars can be met."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as eref                                                   # noqa: E402
import global_coherence_ref as gref                                           # noqa: E402

LD, CLD = gref.LD, gref.CLD


def _exact_pairs_hold(m):
    """A U = U diag(values) with zero error, evaluated in extended precision on the unnormalised vectors (entries 0, +-1, +-i)"""
    A, U = m.A.astype(CLD), m.U.astype(CLD)
    assert np.array_equal(A @ U, U * m.values.astype(LD))
    assert np.array_equal((U.conj().T @ U).real, np.diag(m.n).astype(LD)) and not (U.conj().T @ U).imag.any()


@pytest.mark.parametrize("C", [1, 2, 3, 5, 17, 33, 48, 64, 100, 130, 300])
def test_exact_family_is_exact(C):
    m = gref.exact(C, 1000 + C)
    assert np.array_equal(m.A, m.A.conj().T)
    assert np.array_equal(m.A.astype(np.complex64).astype(np.complex128), m.A), "float32 does not hold an entry"
    assert sorted(m.n) == sorted(n for n in gref.blocks_of(C) for _ in range(n))
    _exact_pairs_hold(m)
    for scale in (2.0 ** -90, 2.0 ** 44):
        s = gref.exact(C, 1000 + C, scale=scale)
        assert np.array_equal(s.A, m.A * scale) and np.array_equal(s.values, m.values * scale)
        assert np.array_equal((s.A * gref.N_OBS).astype(np.complex64).astype(np.complex128), s.A * gref.N_OBS)
        _exact_pairs_hold(s)


def test_exact_family_takes_a_multiset():
    lam = gref.with_multiplicities(64, 3)
    assert sorted(np.unique(lam, return_counts=True)[1])[-3:] == [2, 4, 16]
    m = gref.exact(64, 5, eigenvalues=lam)
    assert sorted(m.values) == sorted(lam)
    _exact_pairs_hold(m)
    g = gref.exact(48, 6, eigenvalues=gref.graded(48))
    assert g.values.max() == 1.0 and g.values.min() == 2.0 ** -40
    _exact_pairs_hold(g)                                                      # (float64 holds these entries; float32 does not)


def test_special_matrices():
    for name, make in gref.SPECIAL.items():
        for C in (6, 32, 40):
            A = make(C)
            assert A.shape == (C, C) and np.array_equal(A, A.conj().T), name
            assert np.linalg.eigvalsh(A).min() > -1e-12 * np.abs(A).max() * C, name
    assert (np.diag(gref.dead_channel(6)) == 0).sum() == 1
    sub = np.diag(gref.imaginary_subdiagonal(6), -1)
    assert not sub.real.any() and sub.imag.all()
    assert np.linalg.matrix_rank(gref.free(20, 8, 1)) == 8


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("C", [3, 17, 40])
def test_record_round_trips(C, dtype, two_sided):
    mats = np.array([[gref.exact(C, 10 * g + f).A for f in range(3)] for g in range(2)])
    rec, stack = gref.record(mats, 8, dtype, two_sided)
    lay = eref.layout(C, eref.PLANE_CSM)
    assert rec.shape == (6, lay.floats_per_bin) and rec.dtype == dtype
    assert np.array_equal(gref.unpack(rec, C, 2, 8), mats)
    N = 3 if two_sided else 4
    assert stack.shape == (2, N, C, C)
    assert np.array_equal(stack[:, :3], mats)
    if not two_sided:
        assert np.array_equal(stack[:, 3], mats[:, 1].conj())
    # the cast changes nothing: the float and the double record hold the same numbers
    assert np.array_equal(rec.astype(np.float64), gref.record(mats, 8, np.float64, two_sided)[0])


def test_record_with_an_inexact_division():
    """n_obs = 12: the stack is what the division of the stored numbers gives, not the matrix that went in"""
    mats = gref.free(5, 12, 3)[None, None]
    rec, stack = gref.record(mats, 12, np.float64, True)
    assert np.array_equal(gref.unpack(rec, 5, 1, 12), stack)
    assert np.abs(stack - mats).max() <= 2.0 ** -52 * np.abs(mats).max()


def test_exact_products():
    """matmul_ld against a plain extended-precision product, at the three amplitudes of the suite"""
    rng = np.random.default_rng(0)
    for scale in (1.0, 2.0 ** -90, 2.0 ** 44):
        X = (rng.standard_normal((40, 40)) + 1j * rng.standard_normal((40, 40))) * scale
        Y = np.linalg.qr(rng.standard_normal((40, 7)) + 1j * rng.standard_normal((40, 7)))[0]
        re, im = gref.cmatmul_ld(X, Y)
        want = X.astype(CLD) @ Y.astype(CLD)
        bound = 2.0 ** -58 * np.abs(X).max()
        assert np.abs(re - want.real).max() <= bound and np.abs(im - want.imag).max() <= bound


def test_check_sees_what_it_should():
    m = gref.exact(16, 9)
    order = np.argsort(m.values)[::-1]
    V = (m.U / np.sqrt(m.n))[:, order]
    V = V * (np.conj(V[0]) / np.abs(V[0]))                                    # row 0 real and positive: every modulus is 1 / 4
    lam = m.values[order]
    r = gref.check(m.A, lam, V, False, m.values)
    assert r["values"] == 0 and r["residual"] <= 4 and r["gram"] <= 4 and r["phase"] <= 1, r
    assert gref.check(m.A, lam[:3][::-1], V[:, :3][:, ::-1], True, m.values)["values"] == 0
    assert gref.check(m.A, lam * (1 + 1e-12), V, False, m.values)["values"] > 1000
    W = V.copy()
    W[:, 2] = (W[:, 2] + 1e-10 * W[:, 3]) / np.sqrt(1 + 1e-20)
    r = gref.check(m.A, lam, W, False, m.values)
    assert r["gram"] > 1e5 and r["residual"] > 10
    assert gref.check(m.A, lam, V * np.exp(1e-9j), False, m.values)["phase"] > 1e5
    F = gref.free(7, 14, 2)
    w, Q = np.linalg.eigh(F)
    top = np.abs(Q).argmax(axis=0)
    Q = Q * (np.conj(Q[top, np.arange(7)]) / np.abs(Q[top, np.arange(7)]))
    assert not gref.over_the_bars(gref.check(F, w[::-1], Q[:, ::-1], False), dict(gref.BARS, phase=8.0))
    with pytest.raises(AssertionError):                                       # the largest component negative
        gref.check(F, w[::-1], -Q[:, ::-1], False)
    with pytest.raises(AssertionError):
        gref.check(m.A, -lam, V, False, m.values)


def numpy_ratios(family, C):
    """the worst ratios of numpy.linalg.eigh (float64) over the matrices of a case of (a), every eigenpair, largest first"""
    mats, vals = gref.cases_a(family, C)
    worst = {}
    for g in range(mats.shape[0]):
        for f in range(mats.shape[1]):
            w, V = np.linalg.eigh(mats[g, f])
            V = V[:, ::-1]
            m = np.abs(V).argmax(axis=0)
            V = V * (np.conj(V[m, np.arange(C)]) / np.abs(V[m, np.arange(C)]))
            r = gref.check(mats[g, f], np.maximum(w[::-1], 0.0), V, False, None if vals is None else vals[g, f])
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    return worst


@pytest.mark.parametrize("C", gref.SIZES)
@pytest.mark.parametrize("family", gref.FAMILIES)
def test_numpy_meets_the_bars(family, C):
    r = numpy_ratios(family, C)
    print(f"\n  {family} C = {C}: " + ", ".join(f"{k} {v:.2f}" for k, v in r.items()))
    bars = dict(gref.BARS, phase=8.0)       # (NumPy's vectors are rotated here in float64 by a complex product: one rounding more)
    assert not gref.over_the_bars(r, bars), r
