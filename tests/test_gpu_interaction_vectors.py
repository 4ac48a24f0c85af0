"""The vectors that attain the maximized imaginary coherence on the device (sc_imaginary_interaction_vectors_f64 through
Connectivity.maximized_imaginary_coherence_vectors) against the NumPy float64 reference of tests/interaction_vectors_ref.py.

Exact spectra go in as uploaded Fourier coefficients whose taper average is S(f) (conditional_granger_ref.coefficients_for), 17
bins a case.  Bounds: those of tests/test_gpu_imaginary_interaction.py for the values and the identities (1e-9 on the float64
engine, 1e-4 on the float32 engines), times the first-order eigenvector amplification max(1, 2 s1 / (s1^2 - s2^2)) of the
REFERENCE's singular values for the vectors themselves (interaction_vectors_ref.amplification).  Every vector comparison prints
its worst error / bound ratio (pytest -s): profiles/interaction_vectors_accuracy.txt."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import conditional_granger_ref as cref
import interaction_vectors_ref as vref
from test_gpu_imaginary_interaction import bounds, lagged_series, multitaper

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_group_sizes", "test_three_uneven_groups_string_labels", "test_mixed_tiers_in_one_launch",
                       "test_trials_tapers_keeps_the_axes", "test_invariance_on_device", "test_real_coefficients_give_zero_and_no_vectors",
                       "test_torch_free_host_gives_the_same_arrays")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FREQ = 17
INTERIOR = range(1, N_FREQ - 1)


def device(S, expectation_type="tapers"):
    import spectral_connectivity_amd as sc
    return sc.Connectivity(cref.coefficients_for(S), expectation_type=expectation_type)


@functools.lru_cache(maxsize=None)
def size_reference(sizes):
    """Spectrum and reference of a group-size case, computed once for the three engines."""
    S, labels, ga, gb = vref.size_case(sizes)
    return S, labels, (ga, gb), vref.vectors(S[:N_FREQ], labels)


def blocks(S, ma, mb):
    return S[np.ix_(ma, ma)].real, S[np.ix_(mb, mb)].real, S[np.ix_(ma, mb)].imag


def check_identities(S, res, atol, rtol, what, interior=INTERIOR):
    """(ii), (v) and the layout, at every bin and pair of ``res`` (arrays already reshaped to [F, G, G(, n)]); S [F, C, C] exact."""
    mic, filters, patterns, members = res
    G = len(members)
    for f in range(mic.shape[0]):
        for i in range(G):
            assert np.isnan(mic[f, i, i]) and np.isnan(filters[f, i, i]).all() and np.isnan(patterns[f, i, i]).all()
            for j in range(i + 1, G):
                ma, mb = members[i], members[j]
                na, nb = len(ma), len(mb)
                Ra, Rb, I = blocks(S[f], ma, mb)
                alpha, beta = filters[f, i, j, :na], filters[f, j, i, :nb]
                pa, pb = patterns[f, i, j, :na], patterns[f, j, i, :nb]
                m = mic[f, i, j]
                assert m == mic[f, j, i] and np.isfinite(m), (what, f, i, j)
                assert np.isnan(filters[f, i, j, na:]).all() and np.isnan(filters[f, j, i, nb:]).all(), (what, f)
                assert np.isnan(patterns[f, i, j, na:]).all() and np.isnan(patterns[f, j, i, nb:]).all(), (what, f)
                vecs = np.r_[alpha, beta, pa, pb]
                if np.isnan(vecs).any():                     # only where the cross block is exactly 0: never inside the band
                    assert np.isnan(vecs).all() and m == 0.0 and f not in interior and np.abs(I).max() <= atol, (what, f, i, j)
                    continue
                nI = np.linalg.norm(I, 2)
                for v, R in ((alpha, Ra), (beta, Rb)):
                    assert abs(v @ R @ v - 1) <= atol * max(1.0, (v @ v) * np.linalg.norm(R, 2)) + rtol, (what, f, i, j)
                na_, nb_ = np.linalg.norm(alpha), np.linalg.norm(beta)
                assert abs(alpha @ I @ beta - m) <= atol * max(1.0, na_ * nI * nb_) + rtol * m, (what, f, i, j)
                assert np.abs(I @ beta - m * pa).max() <= atol * max(1.0, nI * nb_) + rtol * np.abs(m * pa).max(), (what, f, i, j)
                assert np.abs(I.T @ alpha - m * pb).max() <= atol * max(1.0, nI * na_) + rtol * np.abs(m * pb).max(), (what, f, i, j)
                assert np.abs(Ra @ alpha - pa).max() <= (atol + rtol) * max(1.0, np.abs(pa).max()), (what, f, i, j)
                assert np.abs(Rb @ beta - pb).max() <= (atol + rtol) * max(1.0, np.abs(pb).max()), (what, f, i, j)
                assert pa[int(np.argmax(np.abs(pa)))] > 0, (what, "sign rule", f, i, j)
                if f in interior:
                    assert alpha @ I @ beta >= 0, (what, f, i, j)


def check_against_reference(res, ref, atol, what, pairs=None):
    """(iii) at the interior bins: |vector - reference| <= atol max(1, 2 s1 / (s1^2 - s2^2)) max|reference vector|, the singular
    values from the reference.  Prints and returns the worst error / bound."""
    mic, filters, patterns, members = res
    G = len(members)
    worst = 0.0
    for f in INTERIOR:
        for i in range(G):
            for j in range(G):
                if i == j or (pairs is not None and (min(i, j), max(i, j)) not in pairs):
                    continue
                n = len(members[i])
                amp = float(vref.amplification(ref["mic"][f, i, j], ref["sigma2"][f, i, j]))
                for name, got in (("filters", filters), ("patterns", patterns)):
                    want = ref[name][f, i, j, :n]
                    worst = max(worst, np.abs(got[f, i, j, :n] - want).max() / (atol * amp * np.abs(want).max()))
    print(f"interaction vectors accuracy: {what}: worst error / bound = {worst:.3e}")
    return worst


def unpack(out, n_freq=N_FREQ):
    G, n = out.mic.shape[-1], out.filters.shape[-1]
    return (out.mic.reshape(n_freq, G, G), out.filters.reshape(n_freq, G, G, n), out.patterns.reshape(n_freq, G, G, n), out.members)


def test_lds_edge_is_where_the_size_cases_put_it():
    from spectral_connectivity_amd import _lib
    lib = _lib.load()
    e = vref.LDS_EDGE
    assert lib.sc_interaction_vectors_lds_group(e) == e and lib.sc_interaction_vectors_lds_group(e + 1) <= e
    assert (e, e) in vref.GROUP_SIZES and (e, e + 1) in vref.GROUP_SIZES
    assert lib.sc_interaction_vectors_lds_group(128) >= 1 and lib.sc_interaction_vectors_lds_group(129) == 0


@pytest.mark.parametrize("sizes", vref.GROUP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_group_sizes(sizes, _engine_precision):
    """Every tier edge of the MIC kernels and the LDS / scratch edge of the vector kernel, permuted labels."""
    S, labels, g, ref = size_reference(sizes)
    c = device(S)
    out = c.maximized_imaginary_coherence_vectors(labels)
    atol, rtol = bounds(_engine_precision)
    na, nb = sizes
    assert out.mic.shape == (1, 1, N_FREQ, 2, 2) and out.filters.shape == out.patterns.shape == (1, 1, N_FREQ, 2, 2, max(sizes))
    assert out.filters.dtype == out.patterns.dtype == out.mic.dtype == np.float64
    assert list(out.labels) == [0, 1] and [list(m) for m in out.members] == [list(m) for m in ref["members"]]
    # (i) the value is the one of maximized_imaginary_coherence
    mic0, _ = c.maximized_imaginary_coherence(labels)
    assert np.array_equal(np.isnan(out.mic), np.isnan(mic0))
    ok = ~np.isnan(mic0)
    assert (np.abs(out.mic[ok] - mic0[ok]) - (atol + rtol * np.abs(mic0[ok]))).max() <= 0
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, f"{sizes}")                                   # (ii), (v)
    worst = check_against_reference(res, ref, atol, f"{_engine_precision} {na}x{nb}")            # (iii)
    assert worst <= 1.0, f"{sizes}: vectors off the reference by {worst:.3e} x the bound"
    for f in INTERIOR:                                                                          # (iv)
        for (i, j), gv in (((0, 1), g[0]), ((1, 0), g[1])):
            m = out.members[i]
            p = res[2][f, i, j, :len(m)]
            assert abs(p @ gv[m]) / np.linalg.norm(p) >= 0.99, (sizes, f)


def test_three_uneven_groups_string_labels(_engine_precision):
    """Unsorted string labels, groups of 1, 20 and 7 channels: shapes, NaN padding, members, both orders of every pair."""
    rng = np.random.default_rng(5)
    labels = np.array(["v1"] * 1 + ["pfc"] * 20 + ["lgn"] * 7)[rng.permutation(28)]
    S, _, _ = vref.planted_spectrum(labels, 5, pair=(0, 1))                 # planted between lgn (7) and pfc (20)
    c = device(S)
    out = c.maximized_imaginary_coherence_vectors(labels)
    assert list(out.labels) == ["lgn", "pfc", "v1"]
    assert out.mic.shape == (1, 1, N_FREQ, 3, 3) and out.filters.shape == out.patterns.shape == (1, 1, N_FREQ, 3, 3, 20)
    assert [len(m) for m in out.members] == [7, 20, 1]
    for lab, m in zip(out.labels, out.members):
        assert np.array_equal(m, np.flatnonzero(labels == lab))
    atol, rtol = bounds(_engine_precision)
    mic0, _ = c.maximized_imaginary_coherence(labels)
    ok = ~np.isnan(mic0)
    assert np.array_equal(np.isnan(out.mic), ~ok) and (np.abs(out.mic[ok] - mic0[ok]) - (atol + rtol * np.abs(mic0[ok]))).max() <= 0
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, "uneven")      # (every pair, both orders, the padding and the diagonal)
    ref = vref.vectors(S[:N_FREQ], labels)
    assert vref.relative_gap(ref["mic"][1:-1, 0, 1], ref["sigma2"][1:-1, 0, 1]).min() >= 0.3
    assert check_against_reference(res, ref, atol, f"{_engine_precision} uneven 7x20", pairs={(0, 1)}) <= 1.0
    # a single channel against a group: the trivial side is 1 / sqrt(R) and sqrt(R), up to the pair's sign
    v1 = out.members[2][0]
    r = S[:N_FREQ, v1, v1].real
    for f in INTERIOR:
        assert abs(abs(res[1][f, 2, 0, 0]) - 1 / np.sqrt(r[f])) <= (atol + rtol) * 2 and abs(abs(res[2][f, 2, 0, 0]) - np.sqrt(r[f])) <= (atol + rtol) * 2


def test_mixed_tiers_in_one_launch(_engine_precision):
    """Groups of 10, 12 and 60 channels: the pair (10, 12) keeps its blocks in LDS, the pairs with the group of 60 in the scratch."""
    from spectral_connectivity_amd import _lib
    assert 12 <= _lib.load().sc_interaction_vectors_lds_group(60) < 60
    rng = np.random.default_rng(82)
    labels = np.r_[np.zeros(10, int), np.ones(12, int), np.full(60, 2)][rng.permutation(82)]
    S, _, _ = vref.planted_spectrum(labels, 82, pair=(0, 2))
    out = device(S).maximized_imaginary_coherence_vectors(labels)
    atol, rtol = bounds(_engine_precision)
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, "mixed")
    ref = vref.vectors(S[:N_FREQ], labels)
    ok = ~np.isnan(ref["mic"])
    assert (np.abs(res[0][ok] - ref["mic"][ok]) - (atol + rtol * ref["mic"][ok])).max() <= 0
    assert vref.relative_gap(ref["mic"][1:-1, 0, 2], ref["sigma2"][1:-1, 0, 2]).min() >= 0.3
    assert check_against_reference(res, ref, atol, f"{_engine_precision} mixed 10x60", pairs={(0, 2)}) <= 1.0


def test_trials_tapers_keeps_the_axes(_engine_precision):
    S, labels, _, ref = size_reference((2, 3))
    out = device(S, "trials_tapers").maximized_imaginary_coherence_vectors(labels)
    assert out.mic.shape == (1, N_FREQ, 2, 2) and out.filters.shape == out.patterns.shape == (1, N_FREQ, 2, 2, 3)
    atol, rtol = bounds(_engine_precision)
    res = unpack(out)
    check_identities(S[:N_FREQ], res, atol, rtol, "trials_tapers")
    assert check_against_reference(res, ref, atol, f"{_engine_precision} trials_tapers 2x3") <= 1.0


def test_real_coefficients_give_zero_and_no_vectors(caplog, _engine_precision):
    """Purely instantaneous mixing: MIC exactly 0, no direction singled out, and that is no failure."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(9)
    coef = rng.standard_normal((1, 1, 12, 16, 6)).astype(complex)
    with caplog.at_level(logging.WARNING):
        out = sc.Connectivity(coef, expectation_type="tapers").maximized_imaginary_coherence_vectors(np.array([0, 0, 1, 1, 2, 2]))
    off = ~np.eye(3, dtype=bool)
    assert np.all(out.mic[..., off] == 0.0) and np.isnan(out.mic[..., ~off]).all()
    assert np.isnan(out.filters).all() and np.isnan(out.patterns).all()
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and r.name.startswith("spectral_connectivity_amd")]


def test_rank_rule(caplog):
    """The input of the MIC test: the group of 7 channels (> 2 x 3 observations) is NaN without device work, one warning."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(2)
    coef = rng.standard_normal((1, 1, 3, 16, 12)) + 1j * rng.standard_normal((1, 1, 3, 16, 12))
    labels = np.array([0, 0, 1, 1, 1] + [2] * 7)
    c = sc.Connectivity(coef, expectation_type="tapers")
    with caplog.at_level(logging.WARNING):
        out = c.maximized_imaginary_coherence_vectors(labels)
    msgs = [r.getMessage() for r in caplog.records if "twice the" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith("imaginary interaction: 1 groups have more channels than twice the 3 observations")
    mic0, _ = c.maximized_imaginary_coherence(labels)
    assert np.array_equal(np.isnan(out.mic), np.isnan(mic0))
    assert out.filters.shape == (1, 1, 9, 3, 3, 7)
    mic, f, p = out.mic.reshape(-1, 3, 3), out.filters.reshape(-1, 3, 3, 7), out.patterns.reshape(-1, 3, 3, 7)
    for v in (f, p):
        assert np.isnan(v[:, 2]).all() and np.isnan(v[:, :, 2]).all()
        assert np.isfinite(v[:, 0, 1, :2]).all() and np.isfinite(v[:, 1, 0, :3]).all() and np.isnan(v[:, 0, 1, 2:]).all()
    assert np.isfinite(mic[:, 0, 1]).all()


def test_not_positive_definite_block(caplog):
    """The input of the MIC test: a channel without power -- the pairs of its group are NaN, one warning with the same count."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(3)
    coef = rng.standard_normal((1, 1, 8, 16, 6)) + 1j * rng.standard_normal((1, 1, 8, 16, 6))
    coef[..., 4] = 0.0
    labels = np.array([0, 0, 1, 1, 2, 2])
    c = sc.Connectivity(coef, expectation_type="tapers")
    with caplog.at_level(logging.WARNING):
        out = c.maximized_imaginary_coherence_vectors(labels)
    msgs = [r.getMessage() for r in caplog.records if "not positive definite" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith(f"imaginary interaction: {2 * 9} group pairs")      # 2 pairs x 9 bins
    mic0, _ = c.maximized_imaginary_coherence(labels)
    assert np.array_equal(np.isnan(out.mic), np.isnan(mic0))
    mic, f, p = out.mic.reshape(-1, 3, 3), out.filters.reshape(-1, 3, 3, 2), out.patterns.reshape(-1, 3, 3, 2)
    assert np.isnan(mic[:, 2, :]).all() and np.isnan(mic[:, :, 2]).all() and np.isfinite(mic[:, 0, 1]).all()
    for v in (f, p):
        assert np.isnan(v[:, 2]).all() and np.isnan(v[:, :, 2]).all() and np.isfinite(v[:, 0, 1]).all() and np.isfinite(v[:, 1, 0]).all()


def test_errors():
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)
    coef = rng.standard_normal((1, 1, 8, 8, 6)) + 1j * rng.standard_normal((1, 1, 8, 8, 6))
    c = sc.Connectivity(coef, expectation_type="tapers")
    with pytest.raises(ValueError, match="at least two groups"):
        c.maximized_imaginary_coherence_vectors([3] * 6)
    with pytest.raises(ValueError, match="one label per signal"):
        c.maximized_imaginary_coherence_vectors([0, 1, 0, 1])
    big = rng.standard_normal((1, 1, 2, 4, 132)) + 1j * rng.standard_normal((1, 1, 2, 4, 132))
    with pytest.raises(ValueError, match="group 'a' has 129 channels"):
        sc.Connectivity(big, expectation_type="tapers").maximized_imaginary_coherence_vectors(["a"] * 129 + ["b"] * 3)
    x = rng.standard_normal((512, 2, 3))
    with pytest.raises(ValueError, match="Connectivity class directly"):
        sc.multitaper_connectivity(x, 200.0, method="maximized_imaginary_coherence_vectors", time_halfbandwidth_product=2,
                                   time_window_duration=0.64)


# ---- invariance: a real invertible mix T_g inside each group maps patterns by T_g and filters by T_g^-T --------------------
INVARIANCE_SEED = 8
INVARIANCE_LABELS = np.array([0, 1, 0, 1, 2, 2])


def invariance_mix():
    rng = np.random.default_rng(INVARIANCE_SEED)
    T = np.zeros((6, 6))
    for lab in range(3):
        idx = np.flatnonzero(INVARIANCE_LABELS == lab)
        T[np.ix_(idx, idx)] = np.eye(len(idx)) + 0.5 * rng.standard_normal((len(idx), len(idx)))
    return T


def invariance_reference():
    """NumPy multitaper estimate (oracle/spectral_oracle.py) of lagged_series and the reference's singular values on it:
    [W, 65, C, C] spectra -> (sigma_1, sigma_2) [W, 65, G, G]."""
    from oracle import spectral_oracle as so
    x = lagged_series(seed=INVARIANCE_SEED)
    coef, _ = so.multitaper_fft(x, fs=200.0, NW=3, n_time_samples_per_window=128)
    S = np.einsum("wrkni,wrknj->wnij", coef, np.conj(coef)) / (coef.shape[1] * coef.shape[2])
    S = S[:, :65]
    refs = [vref.vectors(S[w], INVARIANCE_LABELS) for w in range(S.shape[0])]
    return np.stack([r["mic"] for r in refs]), np.stack([r["sigma2"] for r in refs])


def test_invariance_on_device(_engine_precision):
    import spectral_connectivity_amd as sc
    x = lagged_series(seed=INVARIANCE_SEED)
    T = invariance_mix()
    s1, s2 = invariance_reference()
    with np.errstate(invalid="ignore", divide="ignore"):
        gap_ok = vref.relative_gap(s1, s2) >= 0.3
    gap_ok[:, [0, -1]] = False
    off = ~np.eye(3, dtype=bool)
    share = gap_ok[:, 1:-1][..., off].mean()
    assert share >= 0.5, f"only {share:.2f} of the interior bins have a relative gap of 0.3"
    a = sc.Connectivity.from_multitaper(multitaper(x)).maximized_imaginary_coherence_vectors(INVARIANCE_LABELS)
    b = sc.Connectivity.from_multitaper(multitaper(x @ T.T)).maximized_imaginary_coherence_vectors(INVARIANCE_LABELS)
    assert a.filters.shape == b.filters.shape == s1.shape + (2,)
    tol = 1e-8 if _engine_precision == "dtype" else 2e-3
    amp = vref.amplification(s1, s2)
    worst = 0.0
    for w, f, i, j in zip(*np.nonzero(gap_ok)):
        if i > j:
            continue
        mi, mj = a.members[i], a.members[j]
        Ti, Tj = T[np.ix_(mi, mi)], T[np.ix_(mj, mj)]
        want = (Ti @ a.patterns[w, f, i, j], Tj @ a.patterns[w, f, j, i],
                np.linalg.solve(Ti.T, a.filters[w, f, i, j]), np.linalg.solve(Tj.T, a.filters[w, f, j, i]))
        got = (b.patterns[w, f, i, j], b.patterns[w, f, j, i], b.filters[w, f, i, j], b.filters[w, f, j, i])
        # the mixed estimate obeys the sign rule itself; the mapped vectors take its sign at THEIR largest entry (two entries of
        # nearly the same magnitude may swap places under the mix's rounding: that is a tie of the rule, not an error)
        assert got[0][int(np.argmax(np.abs(got[0])))] > 0
        k = int(np.argmax(np.abs(want[0])))
        s = 1.0 if got[0][k] * want[0][k] >= 0 else -1.0
        for g_, w_ in zip(got, (s * v for v in want)):
            worst = max(worst, np.abs(g_ - w_).max() / (tol * amp[w, f, i, j] * max(1.0, np.abs(w_).max())))
    print(f"interaction vectors invariance: {_engine_precision}: worst error / bound = {worst:.3e} over {int(gap_ok.sum()) // 2} pairs")
    assert worst <= 1.0


# ---- the other host and two ranks: child processes ------------------------------------------------------------------------
def test_torch_free_host_gives_the_same_arrays(_engine_precision):
    S, labels, _, _ = size_reference((16, 17))
    out = device(S).maximized_imaginary_coherence_vectors(labels)
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
out = sc.Connectivity(cref.coefficients_for(S), expectation_type="tapers").maximized_imaginary_coherence_vectors(labels)
np.savez(sys.argv[5], mic=out.mic, filters=out.filters, patterns=out.patterns, labels=out.labels, m0=out.members[0], m1=out.members[1])
assert type(out).__name__ == "InteractionVectors" and out._fields == ("mic", "filters", "patterns", "labels", "members")
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
    for name in ("mic", "filters", "patterns"):
        np.testing.assert_allclose(other[name], getattr(out, name), rtol=1e-12, atol=1e-14, equal_nan=True)
    assert list(other["labels"]) == list(out.labels)
    assert np.array_equal(other["m0"], out.members[0]) and np.array_equal(other["m1"], out.members[1])


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU): the bins split over the ranks, the same arrays as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29587",
                          os.path.join(ROOT, "tools", "check_sharded_interaction_vectors.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sharded interaction vectors OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
