"""Conditional spectral Granger prediction on the device (sc_conditional.hip through
Connectivity.conditional_spectral_granger_prediction) against the NumPy float64 reference of tests/conditional_granger_ref.py.

Exact spectra go in through the public API as uploaded Fourier coefficients [1, 1, K = C, N, C] whose taper average is S(f)
(conditional_granger_ref.coefficients_for).  Bounds: the float64 engine (the package default) is held to atol = rtol = 1e-6 of
the reference -- the two Wilson iterations stop at the same 1e-8 tolerance.  The float32 engines carry the spectrum through
float32 records: ~1e-7 of the largest entry per record element (the pairwise tests' 2e-5 of the maximum Granger value,
conftest.granger_close), and a conditional value is the log of a ratio of prediction-error variances -- Schur complements of
the spectral matrix, whose relative error is that of the records times the spectrum's condition number (<= ~100 for these
VARs) -- so they are held to 1e-4 absolute + 1e-4 relative.  An entry that is NaN on one side only (the `value <= 0 -> NaN`
cut) is allowed where the finite side is below the absolute bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chunked_calls
import conditional_granger_ref as cref
from conftest import granger_close
from oracle import spectral_oracle as so

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain_var():
    A = np.zeros((2, 3, 3))
    A[0, 0, 0], A[0, 1, 0], A[0, 1, 1], A[0, 2, 1], A[0, 2, 2], A[1, 2, 2] = 0.5, 0.6, 0.3, 0.6, 0.2, -0.3
    sigma = np.array([[1.0, 0.2, 0.0], [0.2, 1.0, 0.1], [0.0, 0.1, 1.0]])
    return A, sigma


def random_var(C, seed, scale=0.35):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((1, C, C)) * (rng.random((1, C, C)) < min(0.4, 6.0 / C))
    A *= scale / max(np.abs(np.linalg.eigvals(A[0])).max(), 1e-3)
    L = np.eye(C) + 0.2 * np.tril(rng.standard_normal((C, C)), -1) * (rng.random((C, C)) < min(1.0, 4.0 / C))
    return A, L @ L.T


def bounds(precision):
    return (1e-6, 1e-6) if precision == "dtype" else (1e-4, 1e-4)


def assert_close(got, ref, atol, rtol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    both = ~np.isnan(got) & ~np.isnan(ref)
    err = np.abs(got[both] - ref[both]) - (atol + rtol * np.abs(ref[both]))
    assert both.any() and err.max() <= 0, f"{what}: worst excess {err.max():.3e} (atol {atol}, rtol {rtol})"
    one = np.isnan(got) != np.isnan(ref)
    worst = np.nan_to_num(np.where(one, np.fmax(got, ref), 0.0)).max() if one.any() else 0.0
    assert worst <= atol, f"{what}: an entry NaN on one side only is {worst:.3e} on the other"


def device(S, expectation_type="tapers"):
    import spectral_connectivity_amd as sc
    # [1, 1, K, N, C]: one window, one trial -- "trials_tapers" averages the same K observations as "tapers"
    return sc.Connectivity(cref.coefficients_for(S), expectation_type=expectation_type)


def squeeze(out):
    return out.reshape(out.shape[-3:])


def test_chain_indirect_edge_removed(_engine_precision):
    A, sigma = chain_var()
    S = cref.var_spectrum(A, sigma, 64)
    c = device(S)
    cond = squeeze(c.conditional_spectral_granger_prediction())
    # the reduced problems' statuses: [C dropped signals, 1 group], all converged
    assert c._last_wilson["status"].shape == (3, 1) and (c._last_wilson["status"] == 1).all()
    pair = squeeze(c.pairwise_spectral_granger_prediction())
    atol = bounds(_engine_precision)[0]
    assert np.nan_to_num(cond[:, 2, 0]).max() < atol, "x -> z given y is not zero"
    assert np.nanmax(pair[:, 2, 0]) > 0.1, "pairwise x -> z should show the indirect edge"
    assert np.nanmin(cond[:, 1, 0]) > 0.01 and np.nanmin(cond[:, 2, 1]) > 0.01
    assert np.isnan(cond[:, [0, 1, 2], [0, 1, 2]]).all()
    assert_close(cond, cref.conditional_granger_ding(S), *bounds(_engine_precision), what="chain vs Ding")


def test_integral_identity(_engine_precision):
    A, sigma = random_var(4, 3)
    N = 64
    S = cref.var_spectrum(A, sigma, N)
    got = squeeze(device(S).conditional_spectral_granger_prediction())
    td = cref.time_domain_conditional(S)
    coupled = td > 1e-3
    assert coupled.sum() >= 2
    mean = cref.two_sided_mean(np.nan_to_num(got), N)
    np.testing.assert_allclose(mean[coupled], td[coupled], rtol=0, atol=bounds(_engine_precision)[0])


@pytest.mark.parametrize("C, expectation_type", [(3, "tapers"), (5, "tapers"), (5, "trials_tapers"), (17, "tapers"), (33, "tapers"),
                                                  (64, "tapers"), (65, "tapers"), (65, "trials_tapers"), (129, "tapers")])
def test_sizes_against_reference(C, expectation_type, _engine_precision):
    """The kernel boundaries: register-resident inverse up to 64 reduced signals (65 signals: 64), matrix-core inverse beyond, the
    blocked inverse and products beyond 128 reduced signals (129 signals).  Above 17 the reference computes three dropped signals."""
    A, sigma = random_var(C, 10 + C)
    N = 32
    S = cref.var_spectrum(A, sigma, N)
    dropped = None if C <= 17 else [0, C // 2, C - 1]
    got = squeeze(device(S, expectation_type).conditional_spectral_granger_prediction())
    ref = cref.conditional_granger_closed(S, dropped)
    cols = list(range(C)) if dropped is None else dropped
    assert_close(got[..., cols], ref[..., cols], *bounds(_engine_precision), what=f"{C} signals")
    if C <= 5:
        assert_close(got, cref.conditional_granger_ding(S), *bounds(_engine_precision), what=f"{C} signals vs Ding")
    off = ~np.eye(C, dtype=bool)
    assert np.isfinite(got[:, off]).mean() > 0.3


def test_513_signals_raise(_engine_precision):
    import spectral_connectivity_amd as sc
    coef = np.zeros((1, 1, 1, 4, 513), dtype=complex)
    coef[..., :] = 1.0
    with pytest.raises(ValueError, match="n_signals <= 512"):
        sc.Connectivity(coef, expectation_type="tapers").conditional_spectral_granger_prediction()


def test_two_signals_equal_pairwise_on_estimated_spectra(_engine_precision):
    """Estimated spectra (multitaper transform of a simulated pair on the device, planes-format records on that engine): with two
    signals the conditioning set is empty and the measure is the pairwise one, NaN pattern included.  The two formulas agree where
    the Wilson factor reproduces the spectrum: on N bins its fixed point leaves the lag-N/2 term of G^-1 S G^-H free, so an estimate
    whose autocovariance fills every lag (window = transform length) is factored only to ~2 % and the two measures differ by that
    much in the NumPy reference's own arithmetic; 64-sample windows on 512 bins (lags within N/8) agree to 4e-7 there."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(7)
    T, R = 1024, 4
    x = rng.standard_normal((T, R, 2))
    for t in range(2, T):
        x[t, :, 0] += 0.55 * x[t - 1, :, 0] - 0.4 * x[t - 2, :, 0]
        x[t, :, 1] += 0.5 * x[t - 1, :, 1] + 0.45 * x[t - 1, :, 0]
    m = sc.Multitaper(x, sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=64,
                      n_time_samples_per_step=64, n_fft_samples=512)
    c = sc.Connectivity.from_multitaper(m)
    cond, pair = c.conditional_spectral_granger_prediction(), c.pairwise_spectral_granger_prediction()
    granger_close(cond, pair, 2e-5, what="two signals: conditional vs pairwise")
    assert np.nanmax(cond[..., 1, 0]) > 0.1


def test_estimated_spectra_against_reference(_engine_precision):
    """Five estimated signals through from_multitaper (records of the engine under test, real-input mirroring) against the
    reference on the oracle's own spectra; also a DTF afterwards reuses the cached full factor."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(11)
    T, R, C = 512, 6, 5
    x = rng.standard_normal((T, R, C))
    for t in range(1, T):
        x[t, :, 1] += 0.5 * x[t - 1, :, 0]
        x[t, :, 2] += 0.5 * x[t - 1, :, 1]
        x[t, :, 4] += 0.4 * x[t - 1, :, 3] + 0.3 * x[t - 1, :, 4]
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=128,
              n_time_samples_per_step=128)
    c = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw))
    got = c.conditional_spectral_granger_prediction()
    G = c._mvar_G
    dtf = c.directed_transfer_function()
    assert c._mvar_G is G
    coef, _ = so.multitaper_fft(x, fs=200.0, NW=2, n_time_samples_per_window=128, n_time_samples_per_step=128)
    S = so.expectation_csm_gemm(coef, "trials_tapers")
    ref = cref.conditional_granger_closed(S)
    assert got.shape == ref.shape == dtf.shape
    atol, rtol = bounds(_engine_precision)
    if _engine_precision != "dtype":
        atol, rtol = 3e-4, 3e-4                  # estimated spectra: less well conditioned than the VARs above
    assert_close(got, ref, atol, rtol, what="estimated spectra")


def test_wrapper(_engine_precision):
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(3)
    x = rng.standard_normal((512, 3, 3))
    x[1:, :, 1] += 0.6 * x[:-1, :, 0]
    kw = dict(time_halfbandwidth_product=2, time_window_duration=0.64)
    da = sc.multitaper_connectivity(x, 200.0, method="conditional_spectral_granger_prediction", **kw)
    assert tuple(da.dims) == ("time", "frequency", "source", "target")
    direct = sc.Connectivity.from_multitaper(sc.Multitaper(x, sampling_frequency=200.0, **kw))
    np.testing.assert_allclose(np.asarray(da.values), direct.conditional_spectral_granger_prediction(), rtol=1e-12, equal_nan=True)
    ds = sc.multitaper_connectivity(x, 200.0, method=None, **kw)
    assert "conditional_spectral_granger_prediction" not in ds.data_vars
    assert "pairwise_spectral_granger_prediction" in ds.data_vars


def test_torch_free_host_gives_the_same_values(_engine_precision):
    A, sigma = random_var(6, 21)
    S = cref.var_spectrum(A, sigma, 32)
    got = squeeze(device(S).conditional_spectral_granger_prediction())
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
np.save(sys.argv[4], c.conditional_spectral_granger_prediction())
assert c._last_wilson["status"].shape == (S.shape[-1], 1)
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
        other = squeeze(np.load(op))
    np.testing.assert_allclose(other, got, rtol=1e-9, atol=1e-12, equal_nan=True)


def chunked_and_whole(S):
    """The measure of ONE object with the default workspace bound and with _lib.CONDITIONAL_WORK_BYTES lowered to the library's own
    workspace query for two dropped signals (_lib.conditional_chunk then returns 2), on whichever host the process runs: the two
    results, the statuses of the chunked run and the dropped signals of each sc_conditional_granger_f64 call it made."""
    import ctypes

    from spectral_connectivity_amd import _lib
    c = device(S)
    whole = squeeze(c.conditional_spectral_granger_prediction())
    lib = _lib._handle()
    nbytes = ctypes.c_size_t()
    _lib.check(lib.sc_conditional_granger_workspace_bytes(1, S.shape[-1], S.shape[0], 2, ctypes.byref(nbytes)),
               "sc_conditional_granger_workspace_bytes")
    with chunked_calls.replaced(_lib, "CONDITIONAL_WORK_BYTES", nbytes.value), \
            chunked_calls.spied(lib, "sc_conditional_granger_f64", 10) as calls:
        chunked = squeeze(c.conditional_spectral_granger_prediction())
    return dict(chunked=chunked, whole=whole, status=c._last_wilson["status"], calls=np.array(calls))


def check_chunked(r, S, precision, host):
    """Three calls of 2, 2, 1 dropped signals into one output: against the reference and against the one-call run of the same
    object, both within bounds(); statuses [5 dropped signals, 1 group], all converged."""
    assert list(r["calls"]) == [2, 2, 1], r["calls"]
    assert r["status"].shape == (5, 1) and (r["status"] == 1).all()
    print(f"conditional Granger, {host} host, {precision}: chunked == one call bit for bit:",
          np.array_equal(r["chunked"], r["whole"], equal_nan=True))
    assert_close(r["chunked"], cref.conditional_granger_closed(S), *bounds(precision), what="chunked vs reference")
    assert_close(r["chunked"], r["whole"], *bounds(precision), what="chunked vs one call")


def test_dropped_signals_in_chunks(_engine_precision):
    """Five signals whose dropped signals go in chunks of two: CONDITIONAL_KEEP_OUTPUT and the offsets of the dropped-signal list
    and of n_iter / status, which the 4 GB default bound never exercises."""
    S = cref.var_spectrum(*random_var(5, 15), 32)
    check_chunked(chunked_and_whole(S), S, _engine_precision, "PyTorch")


def test_dropped_signals_in_chunks_on_the_torch_free_host(_engine_precision):
    S = cref.var_spectrum(*random_var(5, 15), 32)
    r = chunked_calls.on_torch_free_host("test_gpu_conditional_granger", "chunked_and_whole", _engine_precision, S=S)
    check_chunked(r, S, _engine_precision, "torch-free")
