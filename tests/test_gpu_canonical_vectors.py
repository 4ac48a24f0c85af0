"""The vectors that attain canonical coherence and its whole spectrum on the device (sc_canonical_coherence_vectors_f64 through
Connectivity.canonical_coherence_vectors) against the NumPy float64 reference of tests/canonical_vectors_ref.py.

Exact spectra go in as uploaded Fourier coefficients whose taper average is S(f) (conditional_granger_ref.coefficients_for), 17
bins a case.  Bounds: those of tests/test_gpu_imaginary_interaction.py for the values and the identities (1e-9 on the float64
engine, 1e-4 on the float32 engines), times the first-order eigenvector amplification max(1, 2 r1 / (r1^2 - r2^2)) of the
REFERENCE's singular values for the vectors themselves.  ``coherence`` is rho_1; Connectivity.canonical_coherence returns rho_1^2
(as the reference and the oracle do), so (i) compares the SQUARE with it, within the bound of the existing canonical-coherence
tests of groups beyond 32 channels: 5e-5 |ref| + 5e-5 max |ref| on the float32 engines (tests/test_gpu_parity.py), 1e-7 |ref| +
1e-9 max |ref| on the float64 engine (tests/test_gpu_fp64.py).  Every vector comparison prints its worst error / bound ratio
(pytest -s): profiles/canonical_vectors_accuracy.txt.

Measured on the MI355X, worst error / bound over all cases: 2.3e-3 on the float64 engine (16 x 16), 1.9e-3 on the float32 engines."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import canonical_vectors_ref as cvref
import conditional_granger_ref as cref
from test_gpu_imaginary_interaction import bounds

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_group_sizes", "test_three_uneven_groups_string_labels", "test_mixed_tiers_in_one_launch",
                       "test_smaller_group_has_the_higher_label", "test_invariance_under_complex_mixing", "test_zero_cross_block_gives_zero_and_no_vectors",
                       "test_torch_free_host_gives_the_same_arrays")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FREQ = 17
INTERIOR = range(1, N_FREQ - 1)
UNALIGNED = ((2, 3), (16, 17), (64, 65))       # the two largest pattern entries differ by >= 0.12 at every interior bin


def device(S):
    import spectral_connectivity_amd as sc
    return sc.Connectivity(cref.coefficients_for(S), expectation_type="trials_tapers")


@functools.lru_cache(maxsize=None)
def size_reference(sizes):
    """Spectrum and reference of a group-size case, computed once for the three engines."""
    S, labels, _, _ = cvref.size_case(sizes)
    return S, labels, cvref.vectors(S[:N_FREQ], labels)


def value_bound(precision):
    """(rtol, floor) of the existing canonical-coherence tests of that engine: err <= rtol |ref| + floor max |ref|."""
    return (1e-7, 1e-9) if precision == "dtype" else (5e-5, 5e-5)


def check_value(out, c, labels, precision):
    """(i) coherence^2 is what canonical_coherence returns, the NaN positions are identical."""
    cc, lab = c.canonical_coherence(labels)
    assert np.array_equal(lab, out.labels) and cc.shape == out.coherence.shape
    assert np.array_equal(np.isnan(out.coherence), np.isnan(cc))
    ok = ~np.isnan(cc)
    rtol, floor = value_bound(precision)
    assert (np.abs(out.coherence[ok] ** 2 - cc[ok]) - (rtol * np.abs(cc[ok]) + floor * np.abs(cc[ok]).max())).max() <= 0


def unpack(out):
    G, n = out.coherence.shape[-1], out.filters.shape[-1]
    F = out.coherence.shape[0] * out.coherence.shape[1]
    return (out.coherence.reshape(F, G, G), out.coherences.reshape(F, G, G, n), out.filters.reshape(F, G, G, n),
            out.patterns.reshape(F, G, G, n), out.members)


def herm(v):
    return np.conj(v).T


def check_identities(S, res, atol, rtol, what):
    """(ii), (iv) and the layout, at every bin and pair of ``res`` (arrays already reshaped to [F, G, G(, n)]); S [F, C, C] exact.
    The scaling by operand norms is check_identities' of tests/test_gpu_interaction_vectors.py."""
    coh, cohs, filters, patterns, members = res
    G = len(members)
    assert filters.dtype == patterns.dtype == np.complex128 and coh.dtype == cohs.dtype == np.float64
    for f in range(coh.shape[0]):
        for i in range(G):
            assert np.isnan(coh[f, i, i]) and np.isnan(cohs[f, i, i]).all()
            for v in (filters[f, i, i], patterns[f, i, i]):
                assert np.isnan(v.real).all() and np.isnan(v.imag).all()
            for j in range(i + 1, G):
                ma, mb = members[i], members[j]
                na, nb = len(ma), len(mb)
                n_min = min(na, nb)
                Sa, Sb, Sab = S[f][np.ix_(ma, ma)], S[f][np.ix_(mb, mb)], S[f][np.ix_(ma, mb)]
                alpha, beta = filters[f, i, j, :na], filters[f, j, i, :nb]
                pa, pb = patterns[f, i, j, :na], patterns[f, j, i, :nb]
                m = coh[f, i, j]
                assert m == coh[f, j, i] and np.isfinite(m), (what, f, i, j)
                for v, n in ((filters[f, i, j], na), (filters[f, j, i], nb), (patterns[f, i, j], na), (patterns[f, j, i], nb)):
                    assert np.isnan(v[n:].real).all() and np.isnan(v[n:].imag).all(), (what, f)
                    assert np.isfinite(v[:n]).all(), (what, f, i, j)
                cs = cohs[f, i, j]
                assert np.array_equal(cs, cohs[f, j, i], equal_nan=True), (what, f, i, j)
                assert cs[0] == m and np.all(np.diff(cs[:n_min]) <= 0) and np.isnan(cs[n_min:]).all(), (what, f, i, j)
                assert np.all(cs[:n_min] >= 0) and np.all(cs[:n_min] <= 1), (what, f, i, j)
                nS = np.linalg.norm(Sab, 2)
                for v, R in ((alpha, Sa), (beta, Sb)):
                    assert abs(herm(v) @ R @ v - 1) <= atol * max(1.0, (herm(v) @ v).real * np.linalg.norm(R, 2)) + rtol, (what, f, i, j)
                na_, nb_ = np.linalg.norm(alpha), np.linalg.norm(beta)
                assert abs(herm(alpha) @ Sab @ beta - m) <= atol * max(1.0, na_ * nS * nb_) + rtol * m, (what, f, i, j)     # real, >= 0
                assert np.abs(Sab @ beta - m * pa).max() <= atol * max(1.0, nS * nb_) + rtol * np.abs(m * pa).max(), (what, f, i, j)
                assert np.abs(herm(Sab) @ alpha - m * pb).max() <= atol * max(1.0, nS * na_) + rtol * np.abs(m * pb).max(), (what, f, i, j)
                assert np.abs(Sa @ alpha - pa).max() <= (atol + rtol) * max(1.0, np.abs(pa).max()), (what, f, i, j)
                assert np.abs(Sb @ beta - pb).max() <= (atol + rtol) * max(1.0, np.abs(pb).max()), (what, f, i, j)
                # (iv) the phase rule on the device's own output: no margin, no bin skipped
                k = int(np.argmax(np.abs(pa)))
                assert pa[k].real > 0 and abs(pa[k].imag) <= 1e-12 * abs(pa[k]), (what, "phase rule", f, i, j)


def check_against_reference(res, ref, atol, what, pairs=None, aligned=True):
    """(iii) at the interior bins: |e^{i phi} vector - reference| <= atol max(1, 2 r1 / (r1^2 - r2^2)) max|reference vector| for the
    four vectors of a pair with ONE unit phase, the one that best matches the reference pattern of the lower label (aligned=False:
    no phase at all -- the rule must have selected the same entry).  Prints and returns the worst error / bound."""
    _, _, filters, patterns, members = res
    G = len(members)
    r2 = cvref.second(ref["coherences"])
    worst = 0.0
    for f in INTERIOR:
        for i in range(G):
            for j in range(i + 1, G):
                if pairs is not None and (i, j) not in pairs:
                    continue
                na, nb = len(members[i]), len(members[j])
                amp = float(cvref.amplification(ref["coherence"][f, i, j], r2[f, i, j]))
                dot = np.vdot(patterns[f, i, j, :na], ref["patterns"][f, i, j, :na])
                ph = dot / abs(dot) if aligned else 1.0
                for name, got in (("filters", filters), ("patterns", patterns)):
                    for (p, q), n in (((i, j), na), ((j, i), nb)):
                        want = ref[name][f, p, q, :n]
                        worst = max(worst, np.abs(ph * got[f, p, q, :n] - want).max() / (atol * amp * np.abs(want).max()))
    print(f"canonical vectors accuracy: {what}{'' if aligned else ' (no alignment)'}: worst error / bound = {worst:.3e}")
    return worst


def check_coherences(res, ref, atol, rtol, what):
    """(v) every canonical coherence against the reference's singular values, at every bin."""
    ok = ~np.isnan(ref["coherences"])
    assert np.array_equal(np.isnan(res[1]), ~ok), what
    excess = np.abs(res[1][ok] - ref["coherences"][ok]) - (atol + rtol * ref["coherences"][ok])
    assert excess.max() <= 0, (what, excess.max())


@pytest.mark.parametrize("sizes", cvref.GROUP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_group_sizes(sizes, _engine_precision):
    """Every tier edge of the canonical kernels and the LDS / scratch edge of the vector kernel, permuted labels."""
    S, labels, ref = size_reference(sizes)
    c = device(S)
    out = c.canonical_coherence_vectors(labels)
    atol, rtol = bounds(_engine_precision)
    na, nb = sizes
    assert out.coherence.shape == (1, N_FREQ, 2, 2) and out.coherences.shape == (1, N_FREQ, 2, 2, max(sizes))
    assert out.filters.shape == out.patterns.shape == (1, N_FREQ, 2, 2, max(sizes))
    assert list(out.labels) == [0, 1] and [list(m) for m in out.members] == [list(m) for m in ref["members"]]
    assert all(m.dtype == np.int64 for m in out.members)
    check_value(out, c, labels, _engine_precision)                                              # (i)
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, f"{sizes}")                                   # (ii), (iv)
    worst = check_against_reference(res, ref, atol, f"{_engine_precision} {na}x{nb}")            # (iii)
    assert worst <= 1.0, f"{sizes}: vectors off the reference by {worst:.3e} x the bound"
    if sizes in UNALIGNED:                                                                      # (iv), the same entry selected
        worst = check_against_reference(res, ref, atol, f"{_engine_precision} {na}x{nb}", aligned=False)
        assert worst <= 1.0, f"{sizes}: unaligned vectors off the reference by {worst:.3e} x the bound"
    check_coherences(res, ref, atol, rtol, f"{sizes}")                                          # (v)


@pytest.mark.parametrize("sizes", [(3, 2), (17, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smaller_group_has_the_higher_label(sizes, _engine_precision):
    """B on the side of the group with the higher label: the cross block read is S_ba, p and q change roles."""
    S, labels, ref = size_reference(sizes)
    out = device(S).canonical_coherence_vectors(labels)
    atol, rtol = bounds(_engine_precision)
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, f"{sizes}")
    assert check_against_reference(res, ref, atol, f"{_engine_precision} {sizes[0]}x{sizes[1]}") <= 1.0
    check_coherences(res, ref, atol, rtol, f"{sizes}")


def test_lds_edge_is_where_the_size_cases_put_it():
    from spectral_connectivity_amd import _lib
    lib = _lib.load()
    e = cvref.LDS_EDGE
    assert lib.sc_canonical_vectors_lds_group(e) == e and lib.sc_canonical_vectors_lds_group(e + 1) <= e


def test_three_uneven_groups_string_labels(_engine_precision):
    """Unsorted string labels, groups of 1, 20 and 7 channels: shapes, NaN padding, members, both orders of every pair."""
    rng = np.random.default_rng(5)
    labels = np.array(["v1"] * 1 + ["pfc"] * 20 + ["lgn"] * 7)[rng.permutation(28)]
    S, _, _ = cvref.planted_spectrum(labels, 5, pair=(0, 1))                # planted between lgn (7) and pfc (20)
    c = device(S)
    out = c.canonical_coherence_vectors(labels)
    assert type(out).__name__ == "CanonicalVectors"
    assert list(out.labels) == ["lgn", "pfc", "v1"]
    assert out.coherence.shape == (1, N_FREQ, 3, 3) and out.coherences.shape == (1, N_FREQ, 3, 3, 20)
    assert out.filters.shape == out.patterns.shape == (1, N_FREQ, 3, 3, 20)
    assert [len(m) for m in out.members] == [7, 20, 1]
    for lab, m in zip(out.labels, out.members):
        assert np.array_equal(m, np.flatnonzero(labels == lab))
    atol, rtol = bounds(_engine_precision)
    check_value(out, c, labels, _engine_precision)
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, "uneven")      # (every pair, both orders, the padding and the diagonal)
    ref = cvref.vectors(S[:N_FREQ], labels)
    check_coherences(res, ref, atol, rtol, "uneven")
    # every pair: in (lgn, v1) and (pfc, v1) the smaller group has the higher label, B sits on its side
    assert check_against_reference(res, ref, atol, f"{_engine_precision} uneven 7x20x1") <= 1.0
    # a single channel against a group: the trivial side is 1 / sqrt(S_cc) and sqrt(S_cc), up to the pair's phase
    v1 = out.members[2][0]
    r = S[:N_FREQ, v1, v1].real
    for f in INTERIOR:
        assert abs(abs(res[2][f, 2, 0, 0]) - 1 / np.sqrt(r[f])) <= (atol + rtol) * 2 and abs(abs(res[3][f, 2, 0, 0]) - np.sqrt(r[f])) <= (atol + rtol) * 2


def test_mixed_tiers_in_one_launch(_engine_precision):
    """Groups of 10, 12 and 60 channels: the pair (10, 12) keeps its blocks in LDS, the pairs with the group of 60 in the scratch."""
    from spectral_connectivity_amd import _lib
    assert 12 <= _lib.load().sc_canonical_vectors_lds_group(60) < 60
    rng = np.random.default_rng(82)
    labels = np.r_[np.zeros(10, int), np.ones(12, int), np.full(60, 2)][rng.permutation(82)]
    S, _, _ = cvref.planted_spectrum(labels, 82, pair=(0, 2))
    out = device(S).canonical_coherence_vectors(labels)
    atol, rtol = bounds(_engine_precision)
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, "mixed")
    ref = cvref.vectors(S[:N_FREQ], labels)
    check_coherences(res, ref, atol, rtol, "mixed")
    assert check_against_reference(res, ref, atol, f"{_engine_precision} mixed 10x60", pairs={(0, 2)}) <= 1.0


@pytest.mark.parametrize("sizes", [(2, 3), (16, 17), (32, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_total_linear_dependence_is_the_sum_over_the_coherences(sizes):
    """linear_dependence().total = -sum_k ln(1 - rho_k^2), float64 engine.  Bound: an error e <= 1e-9 of every rho_k moves
    -ln(1 - rho_k^2) by 2 rho_k e / (1 - rho_k^2) <= e n_min / (1 - rho_1^2) summed over the n_min terms, to first order
    (rho_1 <= 0.75 on these spectra: a factor <= 2.3 n_min)."""
    from spectral_connectivity_amd import options
    options.precision = "dtype"            # (the package default; the fixture puts the module's selection back afterwards)
    S, labels, ref = size_reference(sizes)
    c = device(S)
    out = c.canonical_coherence_vectors(labels)
    total = c.linear_dependence(labels).total
    assert total.shape == (1, N_FREQ, 2, 2)
    n_min = min(sizes)
    got = -np.log1p(-out.coherences[0, :, 0, 1, :n_min] ** 2).sum(axis=-1)
    bound = 1e-9 * n_min / (1 - out.coherence[0, :, 0, 1] ** 2)
    assert (np.abs(got - total[0, :, 0, 1]) - bound).max() <= 0, np.abs(got - total[0, :, 0, 1]).max()


# ---- invariance: a complex invertible mix A inside one group maps its patterns by A and its filters by A^-H -------------------
def test_invariance_under_complex_mixing(_engine_precision):
    """S' = T S T^H with T = A on the group with label 0, the identity elsewhere: the coherences stay, pattern' = A pattern and
    filter' = A^-H filter for that group, the other group's vectors stay -- all up to the pair's one phase.  Bound: both runs
    are within atol amp max|.| of their exact vectors (iii), element by element; the map multiplies the first run's error by at
    most the infinity norm of the matrix applied."""
    sizes = (16, 17)
    S, labels, ref = size_reference(sizes)
    rng = np.random.default_rng(16)
    m0, m1 = ref["members"]
    A = np.eye(16) + 0.3 * (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))) / 8
    T = np.eye(33, dtype=complex)
    T[np.ix_(m0, m0)] = A
    S2 = T @ S @ herm(T)
    a, b = unpack(device(S).canonical_coherence_vectors(labels)), unpack(device(S2).canonical_coherence_vectors(labels))
    atol, rtol = bounds(_engine_precision)
    ok = ~np.isnan(a[1])
    assert (np.abs(a[1][ok] - b[1][ok]) - 2 * (atol + rtol * a[1][ok])).max() <= 0
    Ainv_h = np.linalg.inv(herm(A))
    r2 = cvref.second(ref["coherences"])
    worst = 0.0
    for f in INTERIOR:
        amp = float(cvref.amplification(ref["coherence"][f, 0, 1], r2[f, 0, 1]))
        maps = ((3, (0, 1), A), (3, (1, 0), None), (2, (0, 1), Ainv_h), (2, (1, 0), None))
        want = [a[k][f, p, q, :len(ref["members"][p])] if X is None else X @ a[k][f, p, q, :16] for k, (p, q), X in maps]
        got = [b[k][f, p, q, :len(ref["members"][p])] for k, (p, q), _ in maps]
        dot = np.vdot(got[0], want[0])
        ph = dot / abs(dot)
        for (k, (p, q), X), g_, w_ in zip(maps, got, want):
            before = np.abs(a[k][f, p, q, :len(ref["members"][p])]).max()
            norm = 1.0 if X is None else np.abs(X).sum(axis=1).max()
            worst = max(worst, np.abs(ph * g_ - w_).max() / (atol * amp * (np.abs(w_).max() + norm * before)))
    print(f"canonical vectors invariance: {_engine_precision}: worst error / bound = {worst:.3e}")
    assert worst <= 1.0


# ---- degenerate inputs ---------------------------------------------------------------------------------------------------------
def package_warnings(caplog):
    return [r for r in caplog.records if r.levelno >= logging.WARNING and r.name.startswith("spectral_connectivity_amd")]


def test_zero_cross_block_gives_zero_and_no_vectors(caplog, _engine_precision):
    """Two independent groups (S_ab = 0 exactly: the Cholesky factor that makes the coefficients keeps the zero pattern):
    coherence 0, every coherence 0, no direction singled out, and that is no failure."""
    S, labels, _ = size_reference((2, 3))
    S = S.copy()
    m0, m1 = np.flatnonzero(labels == 0), np.flatnonzero(labels == 1)
    S[:, m0[:, None], m1[None, :]] = 0
    S[:, m1[:, None], m0[None, :]] = 0
    with caplog.at_level(logging.WARNING):
        out = device(S).canonical_coherence_vectors(labels)
    off = ~np.eye(2, dtype=bool)
    assert np.all(out.coherence[..., off] == 0.0) and np.isnan(out.coherence[..., ~off]).all()
    assert np.all(out.coherences[..., off, :2] == 0.0) and np.isnan(out.coherences[..., off, 2:]).all()
    for v in (out.filters, out.patterns):
        assert np.isnan(v.real).all() and np.isnan(v.imag).all()
    assert not package_warnings(caplog)


def test_group_that_spans_the_observations(caplog):
    """A group with at least as many channels as observations (8 >= 8): coherence 1 with every other group, its coherences 1 up
    to min(n_a, n_b), no vectors; the pair of the two small groups is evaluated."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(2)
    coef = rng.standard_normal((1, 1, 8, 16, 13)) + 1j * rng.standard_normal((1, 1, 8, 16, 13))
    labels = np.array([0, 0, 1, 1, 1] + [2] * 8)
    c = sc.Connectivity(coef, expectation_type="trials_tapers")
    with caplog.at_level(logging.WARNING):
        out = c.canonical_coherence_vectors(labels)
    assert not package_warnings(caplog)
    cc, _ = c.canonical_coherence(labels)
    assert np.array_equal(np.isnan(out.coherence), np.isnan(cc))
    F = out.coherence.shape[1]
    coh, cohs, f, p = out.coherence.reshape(F, 3, 3), out.coherences.reshape(F, 3, 3, 8), out.filters.reshape(F, 3, 3, 8), out.patterns.reshape(F, 3, 3, 8)
    assert np.all(coh[:, 2, :2] == 1.0) and np.all(coh[:, :2, 2] == 1.0)
    for g, n in ((0, 2), (1, 3)):
        assert np.all(cohs[:, 2, g, :n] == 1.0) and np.all(cohs[:, g, 2, :n] == 1.0)
        assert np.isnan(cohs[:, 2, g, n:]).all() and np.isnan(cohs[:, g, 2, n:]).all()
    for v in (f, p):
        assert np.isnan(v[:, 2].real).all() and np.isnan(v[:, :, 2].real).all()
        assert np.isfinite(v[:, 0, 1, :2]).all() and np.isfinite(v[:, 1, 0, :3]).all() and np.isnan(v[:, 0, 1, 2:].real).all()
    assert np.isfinite(coh[:, 0, 1]).all() and np.isfinite(cohs[:, 0, 1, :2]).all() and np.isnan(cohs[:, 0, 1, 2:]).all()
    assert np.abs(coh[:, 0, 1] ** 2 - cc.reshape(F, 3, 3)[:, 0, 1]).max() <= 1e-4


def test_not_positive_definite_block(caplog):
    """A channel without power (the input of the MIC and partial-coherence tests): the pairs of its group are NaN in every
    output, exactly one warning."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(3)
    coef = rng.standard_normal((1, 1, 8, 16, 6)) + 1j * rng.standard_normal((1, 1, 8, 16, 6))
    coef[..., 4] = 0.0
    labels = np.array([0, 0, 1, 1, 2, 2])
    c = sc.Connectivity(coef, expectation_type="trials_tapers")
    with caplog.at_level(logging.WARNING):
        out = c.canonical_coherence_vectors(labels)
    msgs = [r.getMessage() for r in package_warnings(caplog)]
    assert len(msgs) == 1 and "not positive definite" in msgs[0], msgs
    cc, _ = c.canonical_coherence(labels)
    assert np.array_equal(np.isnan(out.coherence), np.isnan(cc))
    F = out.coherence.shape[1]
    coh, cohs, f, p = out.coherence.reshape(F, 3, 3), out.coherences.reshape(F, 3, 3, 2), out.filters.reshape(F, 3, 3, 2), out.patterns.reshape(F, 3, 3, 2)
    assert np.isnan(coh[:, 2, :]).all() and np.isnan(coh[:, :, 2]).all() and np.isfinite(coh[:, 0, 1]).all()
    assert np.isnan(cohs[:, 2]).all() and np.isnan(cohs[:, :, 2]).all() and np.isfinite(cohs[:, 0, 1]).all()
    for v in (f, p):
        assert np.isnan(v[:, 2].real).all() and np.isnan(v[:, :, 2].real).all() and np.isfinite(v[:, 0, 1]).all() and np.isfinite(v[:, 1, 0]).all()


def test_errors():
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)
    coef = rng.standard_normal((1, 1, 8, 8, 6)) + 1j * rng.standard_normal((1, 1, 8, 8, 6))
    c = sc.Connectivity(coef, expectation_type="trials_tapers")
    with pytest.raises(ValueError, match="one label per signal"):
        c.canonical_coherence_vectors([0, 1, 0, 1])
    big = rng.standard_normal((1, 1, 140, 4, 132)) + 1j * rng.standard_normal((1, 1, 140, 4, 132))
    with pytest.raises(ValueError, match="groups of more than 128 channels"):
        sc.Connectivity(big, expectation_type="trials_tapers").canonical_coherence_vectors(["a"] * 129 + ["b"] * 3)
    x = rng.standard_normal((512, 2, 3))
    with pytest.raises(ValueError, match="Connectivity class directly"):
        sc.multitaper_connectivity(x, 200.0, method="canonical_coherence_vectors", time_halfbandwidth_product=2,
                                   time_window_duration=0.64)


# ---- the other host and the sharded class --------------------------------------------------------------------------------------
def test_torch_free_host_gives_the_same_arrays(_engine_precision):
    S, labels, _ = size_reference((16, 17))
    out = device(S).canonical_coherence_vectors(labels)
    code = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import conditional_granger_ref as cref
import spectral_connectivity_amd as sc
from spectral_connectivity_amd import options
options.precision = sys.argv[2]
S, labels = np.load(sys.argv[3]), np.load(sys.argv[4])
out = sc.Connectivity(cref.coefficients_for(S), expectation_type="trials_tapers").canonical_coherence_vectors(labels)
np.savez(sys.argv[5], coherence=out.coherence, coherences=out.coherences, filters=out.filters, patterns=out.patterns, labels=out.labels,
         m0=out.members[0], m1=out.members[1])
assert type(out).__name__ == "CanonicalVectors" and out._fields == ("coherence", "coherences", "filters", "patterns", "labels", "members")
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sp, lp, op = os.path.join(tmp, "S.npy"), os.path.join(tmp, "labels.npy"), os.path.join(tmp, "out.npz")
        np.save(sp, S)
        np.save(lp, labels)
        env = dict(os.environ, SC_HIP_HOST="numpy")
        run = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, sp, lp, op], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0 and "numpy host OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
        other = dict(np.load(op))
    for name in ("coherence", "coherences", "filters", "patterns"):
        got, want = other[name], getattr(out, name)
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert np.array_equal(got.view(np.float64), want.view(np.float64), equal_nan=True), name          # bit-identical
    assert list(other["labels"]) == list(out.labels)
    assert np.array_equal(other["m0"], out.members[0]) and np.array_equal(other["m1"], out.members[1])


def test_sharded_world_size_one_gives_the_same_arrays():
    """parallel.ShardedConnectivity without a process group (one rank holds every trial and every bin)."""
    from spectral_connectivity_amd import parallel
    S, labels, _ = size_reference((16, 17))
    coef = cref.coefficients_for(S)
    one = device(S).canonical_coherence_vectors(labels)
    sharded = parallel.ShardedConnectivity(coef, expectation_type="trials_tapers").canonical_coherence_vectors(labels)
    assert type(sharded).__name__ == "CanonicalVectors"
    for name in ("coherence", "coherences", "filters", "patterns"):
        got, want = getattr(sharded, name), getattr(one, name)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.float64), want.view(np.float64), equal_nan=True), name
    assert list(sharded.labels) == list(one.labels)
