"""tests/mvar_measures_ref.py itself, on the CPU: pinned to the reference's recorded output (golden f9), to the oracle's measure
functions and to the closed forms of its own builders, and the proof that every Tikhonov case of tests/test_gpu_mvar_measures.py
is sensitive to the lam terms at the tolerance that test applies."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvar_measures_ref as mref                                              # noqa: E402
from oracle import spectral_oracle as so                                      # noqa: E402

GOLDEN_NAMES = {"transfer_function": "transfer_function", "mvar_coefficients": "mvar_coefficients", "noise_covariance": "noise_covariance"}
GOLDEN_NAMES.update({m: m for m in mref.MEASURES})


def _global_ratio(got, ref):
    """max |got - ref| / max |ref| over the whole array"""
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("tag", ["var3", "var5"])
def test_golden_f9(golden, tag):
    """From the recorded minimum-phase factor, all eight quantities equal the reference's recorded arrays to 1e-13 of each
    array's maximum (measured: <= 2e-15)."""
    g = golden("f9_mvar")
    got = mref.evaluate(g[f"{tag}__minimum_phase_factor"], "float64")
    assert set(got) == set(mref.QUANTITIES)
    for name in mref.QUANTITIES:
        want = g[f"{tag}__{GOLDEN_NAMES[name]}"]
        assert got[name].shape == want.shape and got[name].dtype == want.dtype, name
        r = _global_ratio(got[name], want)
        print(f"  {tag} {name}: {r:.2e}")
        assert r <= 1e-13, (name, r)


@pytest.mark.parametrize("build,C", [(mref.structured, 7), (mref.free, 12)])
def test_measures_equal_the_oracle(build, C):
    """The five measures are the oracle's functions given the same H, A and Sigma (q=): the same formulas written twice."""
    q = mref.evaluate(build(C, 8, 2, 40 + C), "float64")
    oq = dict(H=q["transfer_function"], A=q["mvar_coefficients"], noise_covariance=q["noise_covariance"])
    for name in mref.MEASURES:
        want = getattr(so, name)(None, q=oq)
        assert want.shape == q[name].shape
        assert _global_ratio(q[name], want) <= 8 * mref.EPS, name
    # and H, A, Sigma are the oracle's own helpers of G
    G = build(C, 8, 2, 40 + C)
    assert _global_ratio(q["transfer_function"], so._take_nonneg(so._transfer_function(G), -3)) <= 64 * mref.EPS
    assert _global_ratio(q["mvar_coefficients"], so._mvar_fourier_coefficients(q["transfer_function"])) <= 64 * mref.EPS
    assert _global_ratio(q["noise_covariance"], so._noise_covariance(G)) <= 64 * mref.EPS


@functools.lru_cache(maxsize=None)
def _closed_case(C, P):
    G, closed = mref.structured(C, 8, P, 300 + C, closed=True)
    return G, closed, mref.evaluate(G, "extended"), mref.evaluate(G, "extended", tikhonov=False)


# 5, 48, 70, 130 with two windows; the sizes of the device test's window cases (three windows) as well: that test adds this
# bar to its own where it compares with the closed form
@pytest.mark.parametrize("C,P", [(5, 2), (48, 2), (70, 2), (130, 2), (5, 3), (48, 3), (64, 3), (100, 3), (130, 3)])
def test_extended_float64_and_closed_forms(C, P):
    """The float64 evaluation equals the extended one to 64 x 2^-52 of each array's maximum (per window; measured: <= 10), and
    the closed forms of ``structured`` hold to the same bar: Sigma = L D^2 L^T, and H = I + B1 z + B2 z^2 for the evaluation
    without the lam terms (with them H moves by lam ||H0^-1|| ~ 1e-8: beyond the bar, as the last assertion shows)."""
    G, closed, ext, ext_plain = _closed_case(C, P)
    f64 = mref.evaluate(G, "float64")
    for name in mref.QUANTITIES:
        r = mref.ratio(f64[name], ext[name])
        print(f"  C = {C} float64 against extended, {name}: {r:.2f}")
        assert r <= 64, (name, r)
    rs, rh = mref.ratio(ext["noise_covariance"], closed["noise_covariance"]), mref.ratio(ext_plain["transfer_function"], closed["transfer_function"])
    print(f"  C = {C} closed forms: Sigma {rs:.2f}, H {rh:.2f}")
    assert rs <= 64 and rh <= 64
    assert mref.ratio(ext["transfer_function"], closed["transfer_function"]) > 64


def test_structured_is_what_the_docstring_says():
    G = mref.structured(20, 8, 2, 9)
    q = mref.evaluate(G, "float64")
    nv = np.einsum("pii->pi", q["noise_covariance"])
    assert nv.max() / nv.min() > 1e4 and nv[1].max() > 4 * nv[0].max() / 10
    assert max(np.linalg.cond(h) for h in q["transfer_function"].reshape(-1, 20, 20)) < 4
    assert np.abs(q["generalized_partial_directed_coherence"] - q["partial_directed_coherence"]).max() > 0.5
    F = mref.free(6, 8, 2, 3)
    assert np.array_equal(F[:, 5], np.conj(F[:, 3])) and not F[:, 0].imag.any() and not F[:, 4].imag.any()


def test_tikhonov_cases_are_sensitive():
    """For every Tikhonov case of the device test the extended result WITHOUT the lam terms misses the device test's own bar
    (K_q x 2^-52 x cond x max |ref| of the window) by a factor of 8 or more IN THE MODIFIED WINDOW, in at least one of the outputs
    that test compares:
    the lam terms are then worth eight tolerances, and dropping them on the device cannot pass."""
    import test_gpu_mvar_measures as tgm
    assert tgm.TIKHONOV_CASES, "no Tikhonov case left"
    for where, C in tgm.TIKHONOV_CASES:
        with_lam, without = tgm.tikhonov_case(where, C)[1:]
        worst = tgm.tikhonov_miss(without, with_lam)
        print(f"  {where} C = {C}: (no-lam - lam) / tolerance: " + ", ".join(f"{n} {v:.1f}" for n, v in worst.items()))
        assert max(worst.values()) >= 8.0, (where, C, worst)
        if where == "h":         # the modified bin is the ill-conditioned one; the others (bin 0 took the compensation) stay tame
            conds = [np.linalg.cond(m.astype(np.complex128)) for m in with_lam["transfer_function"][mref.TIKHONOV_WINDOW]]
            assert 0.5 * mref.TIKHONOV_COND < conds[1] < 2 * mref.TIKHONOV_COND and max(conds[:1] + conds[2:]) < 1e3, conds
