"""Multivariate imaginary coherence on the device (sc_imaginary_interaction_f64 through
Connectivity.maximized_imaginary_coherence / multivariate_interaction_measure) against the NumPy float64 reference of
tests/imaginary_interaction_ref.py.

Exact spectra go in through the public API as uploaded Fourier coefficients [1, 1, K = C, N, C] whose taper average is S(f)
(conditional_granger_ref.coefficients_for of a VAR(1) spectrum).  Bounds: 1e-9 absolute + relative on the float64 engine, 1e-4 on
the float32 engines (float32 records)."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import conditional_granger_ref as cref
import imaginary_interaction_ref as iref

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_exact_spectra", "test_group_sizes", "test_three_uneven_groups_string_labels",
                       "test_invariance_on_device", "test_zero_and_nyquist_bins", "test_torch_free_host_gives_the_same_values")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def var_spectrum(C, seed, n_fft=32):
    """Two-sided spectrum of a well-conditioned VAR(1): sparse coupling of spectral radius 0.5, innovations I + Q Q^T / 2."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((C, C)) * (rng.random((C, C)) < min(0.5, 4.0 / C))
    A *= 0.5 / max(np.abs(np.linalg.eigvals(A)).max(), 1e-3)
    Q = rng.standard_normal((C, C)) / np.sqrt(C)
    return cref.var_spectrum(A[None], np.eye(C) + 0.5 * Q @ Q.T, n_fft)


def bounds(precision):
    return (1e-9, 1e-9) if precision == "dtype" else (1e-4, 1e-4)


def assert_close(got, ref, atol, rtol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN patterns differ"
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok]) - (atol + rtol * np.abs(ref[ok]))
    assert err.max() <= 0, f"{what}: worst excess {err.max():.3e} (atol {atol}, rtol {rtol})"


def device(S, expectation_type="tapers"):
    import spectral_connectivity_amd as sc
    return sc.Connectivity(cref.coefficients_for(S), expectation_type=expectation_type)


def both(c, labels):
    mic, la = c.maximized_imaginary_coherence(labels)
    mim, lb = c.multivariate_interaction_measure(labels)
    assert np.array_equal(la, lb)
    return mic, mim, la


def reference(S, labels):
    n_freq = S.shape[0] // 2 + 1
    return iref.interaction(S[:n_freq], labels)


@pytest.mark.parametrize("expectation_type", ["tapers", "trials_tapers"])
def test_exact_spectra(expectation_type, _engine_precision):
    S = var_spectrum(7, 1)
    labels = [0, 1, 1, 0, 2, 1, 2]
    mic, mim, labs = both(device(S, expectation_type), labels)
    kept = (1, 1) if expectation_type == "tapers" else (1,)
    assert mic.dtype == np.float64 and mim.dtype == np.float64 and list(labs) == [0, 1, 2]
    assert mic.shape == mim.shape == kept + (17, 3, 3)
    ref_mic, ref_mim, _ = reference(S, labels)
    atol, rtol = bounds(_engine_precision)
    assert_close(mic.reshape(ref_mic.shape), ref_mic, atol, rtol, "MIC")
    assert_close(mim.reshape(ref_mim.shape), ref_mim, atol, rtol, "MIM")
    assert np.nanmax(ref_mic[1:-1]) > 0.05


@pytest.mark.parametrize("sizes", [(1, 1), (1, 16), (16, 16), (16, 17), (32, 33), (64, 64), (64, 65), (96, 128), (128, 128)])
def test_group_sizes(sizes, _engine_precision):
    """Every tier and its edges: pair kernel (<= 16 channels), LDS kernel (<= 64), global scratch (<= 128)."""
    na, nb = sizes
    C = na + nb
    S = var_spectrum(C, C)
    labels = np.r_[np.zeros(na, int), np.ones(nb, int)][np.random.default_rng(C).permutation(C)]
    mic, mim, _ = both(device(S), labels)
    ref_mic, ref_mim, _ = reference(S, labels)
    atol, rtol = bounds(_engine_precision)
    assert_close(mic.reshape(ref_mic.shape), ref_mic, atol, rtol, f"MIC {sizes}")
    assert_close(mim.reshape(ref_mim.shape), ref_mim, atol, rtol, f"MIM {sizes}")
    off = mic.reshape(ref_mic.shape)[:, 0, 1]
    assert np.all(off <= 1.0 + 1e-6) and np.all(off ** 2 <= mim.reshape(ref_mim.shape)[:, 0, 1] * (1 + 1e-9) + 1e-15)


def test_three_uneven_groups_string_labels(_engine_precision):
    """Unsorted string labels come back sorted; groups of 1, 20 and 7 channels in one launch (the LDS tier)."""
    S = var_spectrum(28, 5)
    rng = np.random.default_rng(5)
    labels = np.array(["v1"] * 1 + ["pfc"] * 20 + ["lgn"] * 7)[rng.permutation(28)]
    mic, mim, labs = both(device(S), labels)
    assert list(labs) == ["lgn", "pfc", "v1"]
    ref_mic, ref_mim, _ = reference(S, labels)
    atol, rtol = bounds(_engine_precision)
    assert_close(mic.reshape(ref_mic.shape), ref_mic, atol, rtol, "MIC")
    assert_close(mim.reshape(ref_mim.shape), ref_mim, atol, rtol, "MIM")


def multitaper(x, **kw):
    import spectral_connectivity_amd as sc
    kw = dict(dict(sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=128), **kw)
    return sc.Multitaper(x, **kw)


def lagged_series(T=512, R=6, C=6, seed=7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, R, C))
    for t in range(3, T):
        x[t, :, 1] += 0.6 * x[t - 2, :, 0]
        x[t, :, 3] += 0.5 * x[t - 3, :, 2] - 0.3 * x[t - 1, :, 3]
        x[t, :, 5] += 0.4 * x[t - 1, :, 4] + 0.3 * x[t - 2, :, 1]
    return x


def test_singletons_equal_imaginary_coherence():
    """One channel per group on a Multitaper estimate: MIC = |imaginary_coherence()|, MIM its square (float64 engine)."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import options
    options.precision = "dtype"            # (the package default; the fixture puts the module's selection back afterwards)
    x = lagged_series()
    c = sc.Connectivity.from_multitaper(multitaper(x))
    mic, mim, labs = both(c, np.arange(6))
    icoh = np.abs(c.imaginary_coherence())
    assert mic.shape == icoh.shape and list(labs) == list(range(6))
    off = ~np.eye(6, dtype=bool)
    np.testing.assert_allclose(mic[..., off], icoh[..., off], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(mim[..., off], icoh[..., off] ** 2, rtol=1e-10, atol=1e-10)
    assert np.isnan(mic[..., ~off]).all() and np.isnan(mim[..., ~off]).all()
    assert np.nanmax(mic) > 0.2


def test_invariance_on_device(_engine_precision):
    """A real invertible mix of each group's time series leaves both measures unchanged."""
    import spectral_connectivity_amd as sc
    x = lagged_series(seed=8)
    labels = np.array([0, 1, 0, 1, 2, 2])
    rng = np.random.default_rng(8)
    T = np.zeros((6, 6))
    for lab in range(3):
        idx = np.flatnonzero(labels == lab)
        T[np.ix_(idx, idx)] = np.eye(len(idx)) + 0.5 * rng.standard_normal((len(idx), len(idx)))
    a = both(sc.Connectivity.from_multitaper(multitaper(x)), labels)
    b = both(sc.Connectivity.from_multitaper(multitaper(x @ T.T)), labels)
    tol = 1e-8 if _engine_precision == "dtype" else 2e-3
    for got, want, what in ((b[0], a[0], "MIC"), (b[1], a[1], "MIM")):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max() <= tol * max(1.0, np.abs(want[ok]).max()), what


def test_zero_and_nyquist_bins(_engine_precision):
    """Real series: the cross-spectrum is real at the zero and Nyquist bins, so both measures are 0 there (wherever finite);
    real Fourier coefficients (purely instantaneous mixing) give exactly 0 at every bin."""
    import spectral_connectivity_amd as sc
    x = lagged_series(seed=9)
    labels = np.array([0, 0, 1, 1, 2, 2])
    mic, mim, _ = both(sc.Connectivity.from_multitaper(multitaper(x, n_fft_samples=128)), labels)
    assert mic.shape[-3] == 65
    tol = 1e-7 if _engine_precision == "dtype" else 1e-3
    for v in (mic, mim):
        edge = v[..., [0, -1], :, :]
        assert np.nanmax(np.abs(edge)) <= tol and np.isfinite(edge[..., 0, 1]).all()
    assert np.nanmax(mic[..., 1:-1, :, :]) > 0.1
    rng = np.random.default_rng(9)
    coef = rng.standard_normal((1, 1, 12, 16, 6)).astype(complex)
    mic, mim, _ = both(sc.Connectivity(coef, expectation_type="tapers"), labels)
    off = ~np.eye(3, dtype=bool)
    assert np.all(mic[..., off] == 0.0) and np.all(mim[..., off] == 0.0)


def test_errors():
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)
    coef = rng.standard_normal((1, 1, 8, 8, 6)) + 1j * rng.standard_normal((1, 1, 8, 8, 6))
    c = sc.Connectivity(coef, expectation_type="tapers")
    for method in (c.maximized_imaginary_coherence, c.multivariate_interaction_measure):
        with pytest.raises(ValueError, match="at least two groups"):
            method([3] * 6)
        with pytest.raises(ValueError, match="one label per signal"):
            method([0, 1, 0, 1])
    big = rng.standard_normal((1, 1, 2, 4, 132)) + 1j * rng.standard_normal((1, 1, 2, 4, 132))
    with pytest.raises(ValueError, match="group 'a' has 129 channels"):
        sc.Connectivity(big, expectation_type="tapers").maximized_imaginary_coherence(["a"] * 129 + ["b"] * 3)
    x = rng.standard_normal((512, 2, 3))
    for name in ("maximized_imaginary_coherence", "multivariate_interaction_measure"):
        with pytest.raises(ValueError, match="Connectivity class directly"):
            sc.multitaper_connectivity(x, 200.0, method=name, time_halfbandwidth_product=2, time_window_duration=0.64)


def test_rank_rule(caplog):
    """3 observations: a group of 7 channels (> 2 x 3) has a singular real block -- its pairs are NaN without device work, one
    warning; the pair of the groups of 2 and 3 channels is computed."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(2)
    coef = rng.standard_normal((1, 1, 3, 16, 12)) + 1j * rng.standard_normal((1, 1, 3, 16, 12))
    labels = np.array([0, 0, 1, 1, 1] + [2] * 7)
    c = sc.Connectivity(coef, expectation_type="tapers")
    with caplog.at_level(logging.WARNING):
        mic, _ = c.maximized_imaginary_coherence(labels)
    msgs = [r.getMessage() for r in caplog.records if "twice the" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith("imaginary interaction: 1 groups have more channels than twice the 3 observations")
    mim, _ = c.multivariate_interaction_measure(labels)
    for v in (mic, mim):
        v = v.reshape(-1, 3, 3)
        assert np.isnan(v[:, 2, :]).all() and np.isnan(v[:, :, 2]).all() and np.isfinite(v[:, 0, 1]).all()


def test_not_positive_definite_block(caplog):
    """A channel whose coefficients are all zero gives an exactly zero pivot: the pairs of its group are NaN, one warning."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(3)
    coef = rng.standard_normal((1, 1, 8, 16, 6)) + 1j * rng.standard_normal((1, 1, 8, 16, 6))
    coef[..., 4] = 0.0
    labels = np.array([0, 0, 1, 1, 2, 2])
    c = sc.Connectivity(coef, expectation_type="tapers")
    with caplog.at_level(logging.WARNING):
        mic, _ = c.maximized_imaginary_coherence(labels)
    mic = mic.reshape(-1, 3, 3)
    assert np.isnan(mic[:, 2, :]).all() and np.isnan(mic[:, :, 2]).all() and np.isfinite(mic[:, 0, 1]).all()
    msgs = [r.getMessage() for r in caplog.records if "not positive definite" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith(f"imaginary interaction: {2 * 9} group pairs")      # 2 pairs x 9 bins


def test_torch_free_host_gives_the_same_values(_engine_precision):
    S = var_spectrum(9, 21)
    labels = np.array([2, 0, 1, 2, 0, 1, 1, 0, 2])
    mic, mim, _ = both(device(S), labels)
    code = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import conditional_granger_ref as cref
import spectral_connectivity_amd as sc
from spectral_connectivity_amd import options
options.precision = sys.argv[2]
S = np.load(sys.argv[3])
c = sc.Connectivity(cref.coefficients_for(S), expectation_type="tapers")
labels = np.array([2, 0, 1, 2, 0, 1, 1, 0, 2])
mic, la = c.maximized_imaginary_coherence(labels)
mim, lb = c.multivariate_interaction_measure(labels)
np.save(sys.argv[4], np.stack([mic, mim]))
assert list(la) == list(lb) == [0, 1, 2]
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sp, op = os.path.join(tmp, "S.npy"), os.path.join(tmp, "out.npy")
        np.save(sp, S)
        env = dict(os.environ, SC_HIP_HOST="numpy")
        out = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, sp, op], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "numpy host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        other = np.load(op)
    np.testing.assert_allclose(other, np.stack([mic, mim]), rtol=1e-12, atol=1e-14, equal_nan=True)


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU): the bins split over the ranks, the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29563",
                          os.path.join(ROOT, "tools", "check_sharded_interaction.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sharded imaginary interaction OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
