"""The reference of the canonical-values suite (tests/canonical_values_ref.py) checked on the CPU: the ``exact`` family is exactly
Hermitian, positive semi-definite and has the coherences it states, the interaction view gives MIM = sum rho^2, the ``free`` truth
agrees with the plain NumPy reference, and the committed bars are what the rule of tools/canonical_values_accuracy.py gives."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canonical_values_ref as vref                                           # noqa: E402

SIZES = [(1, 1), (1, 2), (3, 5), (16, 16), (16, 17), (33, 20), (64, 65), (97, 128)]


@pytest.mark.parametrize("view", vref.VIEWS)
@pytest.mark.parametrize("sizes", SIZES)
def test_exact_family_has_the_coherences_it_states(sizes, view):
    na, nb = sizes
    rho = vref.distinct_coherences(min(na, nb), 40 + na)
    m = vref.exact(na, nb, rho, 50 + nb, view)
    assert np.array_equal(m.S, m.S.conj().T), "not exactly Hermitian"
    assert (m.kappa <= 8.0 * (1 + 1e-12)).all(), m.kappa
    assert sorted(np.concatenate(m.groups)) == list(range(na + nb)) and [len(g) for g in m.groups] == [na, nb]
    assert any(not np.array_equal(g, np.sort(g)) for g in m.groups) or max(sizes) < 3, "the member lists are sorted"
    sv = vref.numpy_pair(*vref.blocks(m.S, m.groups[0], m.groups[1], view))[0]
    assert np.abs(sv - np.sort(rho)[::-1]).max() <= 16 * vref.EPS, np.abs(sv - np.sort(rho)[::-1]).max() / vref.EPS
    truth = vref.truth_exact(rho)
    got = vref.numpy_values(m.S, m.groups[0], m.groups[1], view)
    for kind, v in got.items():
        assert vref.check(kind, v, truth[kind], min(sizes)) <= vref.BARS[kind]
    if view == "interaction":
        assert abs(got["mim"] - float((rho ** 2).sum())) <= vref.K_MIM * vref.EPS * min(sizes)
        assert got["mic"] ** 2 <= got["mim"] * (1 + 4 * vref.EPS)


@pytest.mark.parametrize("sizes", SIZES)
def test_joint_matrix_is_positive_semi_definite(sizes):
    """[[I, R], [R^T, I]] with 0 <= rho <= 1 between the mixers; rho_1 = 1 makes it singular and both groups stay positive definite"""
    na, nb = sizes
    n = min(sizes)
    for rho in (vref.distinct_coherences(n, 3), np.r_[1.0, np.zeros(n - 1)]):
        m = vref.exact(na, nb, rho, 60 + na, "canonical")
        w = np.linalg.eigvalsh(m.S)
        assert w.min() >= -64 * vref.EPS * w.max(), w.min()
        assert (m.kappa <= 8.0 * (1 + 1e-12)).all()
        if rho[0] == 1.0:
            assert w.min() <= 64 * vref.EPS * w.max()


def test_interaction_view_ignores_the_free_parts():
    m = vref.exact(16, 17, vref.distinct_coherences(16, 1), 2, "interaction")
    bare = vref.exact(16, 17, vref.distinct_coherences(16, 1), 2, "interaction", free_part=False)
    a, b = m.groups
    assert np.abs(m.S[np.ix_(a, b)].real).max() > 0.5 and np.abs(m.S[np.ix_(a, a)].imag).max() > 0.5
    c, d = bare.groups                                    # (the free parts draw from the generator before the permutation does)
    assert not bare.S[np.ix_(c, d)].real.any() and not bare.S[np.ix_(c, c)].imag.any()
    for x, y in zip(vref.blocks(m.S, a, b, "interaction"), vref.blocks(bare.S, c, d, "interaction")):
        assert np.array_equal(x, y)


def test_three_groups_and_an_uncoupled_pair():
    rho = {(0, 1): vref.distinct_coherences(5, 1), (1, 2): vref.distinct_coherences(9, 2)}
    m = vref.exact_groups((5, 16, 9), rho, 3)
    assert np.array_equal(m.S, m.S.conj().T)
    for (a, b), r in rho.items():
        sv = vref.numpy_pair(*vref.blocks(m.S, m.groups[a], m.groups[b], "canonical"))[0]
        assert np.abs(sv - np.sort(r)[::-1]).max() <= 16 * vref.EPS
    assert not m.S[np.ix_(m.groups[0], m.groups[2])].any()


@pytest.mark.parametrize("p", vref.CLUSTER_P)
@pytest.mark.parametrize("n", [16, 17, 64, 65, 128])
def test_cluster_spectra_are_held_exactly(n, p):
    """(the builder asserts that float64 holds every entry)"""
    for view in vref.VIEWS:
        m = vref.cluster_case(n, p, 70 + n, view)
        assert np.array_equal(np.sort(m.rho[(0, 1)]), vref.cluster(n, p))


@pytest.mark.parametrize("name", list(vref.SPECTRA))
def test_spectra_of_the_structure_cases(name):
    for n in (16, 17, 128):
        rho = vref.SPECTRA[name](n)
        assert rho.shape == (n,) and (rho >= 0).all() and (rho <= 1).all()
        vref.exact(n, n, rho, 80 + n, "canonical")
    assert vref.graded(16).min() == 2.0 ** -20 and vref.SPECTRA["rho_1_is_one"](16).max() == 1.0


@pytest.mark.parametrize("sizes", [(1, 2), (3, 5), (16, 17), (64, 65)])
def test_free_truth_agrees_with_the_numpy_reference(sizes):
    for view in vref.VIEWS:
        mats, groups, truths = vref.case_a("free", sizes, view)
        for f in range(mats.shape[0]):
            got = vref.numpy_values(mats[f], groups[0], groups[1], view)
            for kind, v in got.items():
                assert abs(v - float(truths[f][kind])) <= 1e-12, (kind, v, truths[f][kind])


def test_check_units():
    assert vref.check("canonical", 0.25 + 2.0 ** -50, np.longdouble(0.25)) == 4.0
    assert vref.check("mim", 1.0 + 2.0 ** -48, np.longdouble(1.0), n_min=4) == 4.0
    assert vref.check("mic", 0.5 + 2.0 ** -42, np.longdouble(0.5), kappa=1024.0) == 1.0
    with pytest.raises(AssertionError):
        vref.check("mic", np.nan, np.longdouble(0.5))


def test_conditioning_series_has_the_condition_it_states():
    for p in vref.CONDITIONING:
        _, _, _, kappa = vref.conditioning_case((16, 16), p, "canonical")
        assert 2.0 ** p <= kappa <= 2.0 ** (p + 3), (p, kappa)


def test_jacobi_allowance():
    assert vref.jacobi_allowance(16, 16, 16) == pytest.approx(np.sqrt(32e-24) / vref.EPS)
    assert vref.jacobi_allowance(17, 32, 32) < vref.K_CANONICAL < vref.jacobi_allowance(65, 128, 128)


def test_committed_bars_are_what_the_rule_gives():
    """8 x the worst NumPy ratio over the cases of (a), rounded up to a power of two -- the rule of the tool, evaluated here"""
    worst = {}
    for sizes in vref.PAIR_SIZES:
        for family in vref.FAMILIES:
            for k, v in vref.numpy_ratios(family, sizes).items():
                worst[k] = max(v, worst.get(k, 0.0))
    assert {k: vref.bar_from(v) for k, v in worst.items()} == vref.BARS, worst
    worst_c = max(vref.numpy_conditioning_ratio(s, p) for s in vref.CONDITIONING_SIZES for p in vref.CONDITIONING)
    assert vref.bar_from(worst_c) == vref.K_CONDITIONING, worst_c
