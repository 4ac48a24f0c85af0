"""The NumPy reference of the MIC vectors (tests/interaction_vectors_ref.py) against itself, and what the device tests rely on
in the test spectrum: no GPU."""
import numpy as np
import pytest

import interaction_vectors_ref as vref

N_FREQ = 17
INTERIOR = slice(1, N_FREQ - 1)


@pytest.fixture(scope="module", params=vref.GROUP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    S, labels, ga, gb = vref.size_case(request.param)
    S = S[:N_FREQ]
    return dict(sizes=request.param, S=S, labels=labels, g=(ga, gb), ewald=vref.vectors(S, labels, "ewald"),
                cholesky=vref.vectors(S, labels, "cholesky"))


def test_two_forms_agree(case):
    e, c = case["ewald"], case["cholesky"]
    for name in ("mic", "filters", "patterns"):
        a, b = e[name][INTERIOR], c[name][INTERIOR]
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        ok = ~np.isnan(a)
        assert np.abs(a[ok] - b[ok]).max() <= 1e-10 * max(1.0, np.abs(a[ok]).max()), (name, case["sizes"])
    assert np.array_equal(e["labels"], [0, 1]) and [len(m) for m in e["members"]] == list(case["sizes"])


@pytest.mark.parametrize("form", ["ewald", "cholesky"])
def test_identities(case, form):
    r, S = case[form], case["S"]
    ma, mb = r["members"]
    na, nb = len(ma), len(mb)
    for f in range(1, N_FREQ - 1):
        Ra, Rb, I = S[f][np.ix_(ma, ma)].real, S[f][np.ix_(mb, mb)].real, S[f][np.ix_(ma, mb)].imag
        alpha, beta = r["filters"][f, 0, 1, :na], r["filters"][f, 1, 0, :nb]
        pa, pb = r["patterns"][f, 0, 1, :na], r["patterns"][f, 1, 0, :nb]
        mic = r["mic"][f, 0, 1]
        assert abs(alpha @ Ra @ alpha - 1) <= 1e-12 and abs(beta @ Rb @ beta - 1) <= 1e-12
        assert abs(alpha @ I @ beta - mic) <= 1e-12
        assert np.abs(I @ beta - mic * pa).max() <= 1e-12 and np.abs(I.T @ alpha - mic * pb).max() <= 1e-12
        assert np.abs(Ra @ alpha - pa).max() <= 1e-12 and np.abs(Rb @ beta - pb).max() <= 1e-12
        k = int(np.argmax(np.abs(pa)))
        assert pa[k] > 0
        assert np.isnan(r["filters"][f, 0, 1, na:]).all() and np.isnan(r["patterns"][f, 1, 0, nb:]).all()
        assert np.isnan(r["filters"][f, 0, 0]).all() and np.isnan(r["patterns"][f, 1, 1]).all()


def test_spectrum_has_what_the_device_tests_rely_on(case):
    """A well separated sigma_1 at every interior bin, well-conditioned real blocks, and patterns that show the planted vectors."""
    r, S = case["ewald"], case["S"]
    s1, s2 = r["mic"][INTERIOR, 0, 1], r["sigma2"][INTERIOR, 0, 1]
    assert vref.relative_gap(s1, s2).min() >= 0.3, (case["sizes"], vref.relative_gap(s1, s2).min())
    assert s1.min() >= 0.1 and s1.max() <= 0.8, (s1.min(), s1.max())
    assert vref.amplification(s1, s2).max() <= 2.0 / (0.3 * 0.1) + 1
    ma, mb = r["members"]
    for m in (ma, mb):
        assert np.linalg.cond(S[INTERIOR][:, m[:, None], m[None, :]].real).max() < 8
    for f in range(1, N_FREQ - 1):
        for (i, j), m, g in (((0, 1), ma, case["g"][0]), ((1, 0), mb, case["g"][1])):
            p = r["patterns"][f, i, j, :len(m)]
            assert abs(p @ g[m]) / np.linalg.norm(p) >= 0.99, (case["sizes"], f)


def test_sign_rule_takes_the_lowest_index_on_a_tie():
    pa, other = vref.apply_sign_rule(np.array([-2.0, 2.0, 1.0]), np.array([-2.0, 2.0, 1.0]), np.array([1.0, -1.0]))
    assert list(pa) == [2.0, -2.0, -1.0] and list(other) == [-1.0, 1.0]


def test_real_cross_spectrum_gives_zero_and_no_vectors():
    S, labels, _, _ = vref.size_case((2, 3))
    r = vref.vectors(S[:N_FREQ].real + 0j, labels)
    assert np.all(r["mic"][:, 0, 1] == 0.0) and np.isnan(r["filters"]).all() and np.isnan(r["patterns"]).all()
