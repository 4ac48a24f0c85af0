"""The NumPy reference of the canonical-coherence vectors (tests/canonical_vectors_ref.py) against itself, against the linear
dependence reference and the oracle, and what the device tests rely on in the test spectrum: no GPU."""
import numpy as np
import pytest

import canonical_vectors_ref as cvref
import conditional_granger_ref as cref
import linear_dependence_ref as lref

N_FREQ = 17
INTERIOR = slice(1, N_FREQ - 1)


@pytest.fixture(scope="module", params=cvref.GROUP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    S, labels, _, _ = cvref.size_case(request.param)
    S = S[:N_FREQ]
    return dict(sizes=request.param, S=S, labels=labels, ewald=cvref.vectors(S, labels, "ewald"),
                cholesky=cvref.vectors(S, labels, "cholesky"))


def test_two_forms_agree(case):
    e, c = case["ewald"], case["cholesky"]
    amp = cvref.amplification(e["coherence"][INTERIOR, 0, 1], cvref.second(e["coherences"])[INTERIOR, 0, 1]).max()
    for name in ("coherence", "coherences", "filters", "patterns"):
        a, b = e[name][INTERIOR], c[name][INTERIOR]
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        ok = ~np.isnan(a)
        assert np.abs(a[ok] - b[ok]).max() <= 1e-10 * amp * max(1.0, np.abs(a[ok]).max()), (name, case["sizes"])
    assert np.array_equal(e["labels"], [0, 1]) and [len(m) for m in e["members"]] == list(case["sizes"])


@pytest.mark.parametrize("form", ["ewald", "cholesky"])
def test_identities(case, form):
    r, S = case[form], case["S"]
    ma, mb = r["members"]
    na, nb = len(ma), len(mb)
    for f in range(1, N_FREQ - 1):
        Sa, Sb, Sab = S[f][np.ix_(ma, ma)], S[f][np.ix_(mb, mb)], S[f][np.ix_(ma, mb)]
        alpha, beta = r["filters"][f, 0, 1, :na], r["filters"][f, 1, 0, :nb]
        pa, pb = r["patterns"][f, 0, 1, :na], r["patterns"][f, 1, 0, :nb]
        rho = r["coherence"][f, 0, 1]
        assert abs(alpha.conj() @ Sa @ alpha - 1) <= 1e-10 and abs(beta.conj() @ Sb @ beta - 1) <= 1e-10
        assert abs(alpha.conj() @ Sab @ beta - rho) <= 1e-10                     # (real and >= 0: rho is)
        assert np.abs(Sab @ beta - rho * pa).max() <= 1e-10 and np.abs(Sab.conj().T @ alpha - rho * pb).max() <= 1e-10
        assert np.abs(Sa @ alpha - pa).max() <= 1e-10 and np.abs(Sb @ beta - pb).max() <= 1e-10
        k = int(np.argmax(np.abs(pa)))
        assert pa[k].real > 0 and abs(pa[k].imag) <= 1e-15 * abs(pa[k])
        cs = r["coherences"][f, 0, 1]
        assert cs[0] == rho and np.all(np.diff(cs[:min(na, nb)]) <= 0) and np.isnan(cs[min(na, nb):]).all()
        assert np.array_equal(cs, r["coherences"][f, 1, 0], equal_nan=True)
        assert np.isnan(r["filters"][f, 0, 1, na:]).all() and np.isnan(r["patterns"][f, 1, 0, nb:]).all()
        assert np.isnan(r["filters"][f, 0, 0]).all() and np.isnan(r["patterns"][f, 1, 1]).all() and np.isnan(r["coherences"][f, 0, 0]).all()


@pytest.mark.parametrize("sizes", [(2, 3), (16, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_total_linear_dependence_from_the_coherences(sizes):
    S, labels, _, _ = cvref.size_case(sizes)
    S = S[:N_FREQ]
    r = cvref.vectors(S, labels, "cholesky")
    total = lref.dependence(S, labels)[0]
    n_min = min(sizes)
    got = -np.log1p(-r["coherences"][:, 0, 1, :n_min] ** 2).sum(axis=-1)
    assert np.abs(got - total[:, 0, 1]).max() <= 1e-10


@pytest.mark.parametrize("sizes", [(2, 3), (16, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_coherence_is_the_oracles_canonical_coherence(sizes):
    """The oracle (as the reference and Connectivity.canonical_coherence) returns the SQUARED largest singular value."""
    from oracle import spectral_oracle as so
    S, labels, _, _ = cvref.size_case(sizes)
    ref, ref_labels = so.canonical_coherence(cref.coefficients_for(S), labels)
    r = cvref.vectors(S[:N_FREQ], labels)
    assert np.array_equal(ref_labels, r["labels"]) and ref.shape == (1, N_FREQ, 2, 2)
    assert np.abs(r["coherence"][:, 0, 1] ** 2 - ref[0, :, 0, 1]).max() <= 1e-10


def test_spectrum_has_what_the_device_tests_rely_on(case):
    r, S = case["ewald"], case["S"]
    s1, s2 = r["coherence"][INTERIOR, 0, 1], cvref.second(r["coherences"])[INTERIOR, 0, 1]
    assert s1.min() >= 0.63 and s1.max() <= 0.75, (case["sizes"], s1.min(), s1.max())
    assert cvref.amplification(s1, s2).max() <= 4.4, (case["sizes"], cvref.amplification(s1, s2).max())
    assert np.linalg.cond(S[INTERIOR]).max() <= 9.15                           # (9.143 at (1, 16), bin 15: the largest)


def test_phase_rule():
    pa = np.array([1j, -2.0, 2j, 0.5])
    once = cvref.apply_phase_rule(pa, pa, np.array([1.0, 1j]))
    assert np.allclose(once[0], [-1j, 2.0, -2j, -0.5]) and np.allclose(once[1], [-1.0, -1j])      # the lowest index on the tie
    twice = cvref.apply_phase_rule(once[0], *once)
    for a, b in zip(once, twice):
        assert np.array_equal(a, b)                                                                # idempotent


def test_phase_rule_is_idempotent_on_the_reference(case):
    r = case["cholesky"]
    na = case["sizes"][0]
    for f in range(1, N_FREQ - 1):
        pa, alpha = r["patterns"][f, 0, 1, :na], r["filters"][f, 0, 1, :na]
        again = cvref.apply_phase_rule(pa, pa, alpha)
        assert np.abs(again[0] - pa).max() <= 1e-15 * np.abs(pa).max() and np.abs(again[1] - alpha).max() <= 1e-15 * np.abs(alpha).max()


def test_zero_cross_block_gives_zero_and_no_vectors():
    S, labels, _, _ = cvref.size_case((2, 3))
    S = S[:N_FREQ].copy()
    a, b = np.flatnonzero(labels == 0), np.flatnonzero(labels == 1)
    S[:, a[:, None], b[None, :]] = 0
    S[:, b[:, None], a[None, :]] = 0
    r = cvref.vectors(S, labels)
    assert np.all(r["coherence"][:, 0, 1] == 0.0) and np.all(r["coherences"][:, 0, 1, :2] == 0.0) and np.isnan(r["coherences"][:, 0, 1, 2:]).all()
    assert np.isnan(r["filters"]).all() and np.isnan(r["patterns"]).all()
