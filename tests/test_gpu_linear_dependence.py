"""Total, instantaneous and lagged linear dependence on the device (sc_linear_dependence_f64 through
Connectivity.linear_dependence / lagged_coherence) against the NumPy float64 reference of tests/linear_dependence_ref.py.

Exact spectra go in through the public API as uploaded Fourier coefficients [1, 1, K = C, N, C] whose taper average is S(f)
(conditional_granger_ref.coefficients_for of the VAR(1) spectra of the MIC tests, 17 bins).  Bounds per output,
atol + rtol |ref|: 1e-9 for both on the float64 engine, 1e-4 for both on the float32 engines (float32 records) -- the MIC tests'.

total = instantaneous + lagged on the device: the group kernel forms the lagged part as that difference in float64, so the sum
gives the total back to one rounding of each operation; the pairwise kernel evaluates three closed forms, each elementary
function within a few units of 2^-52 of values of order 1 ... 10.  Both are held to 1e-12 (1 + |total|), some hundred times
that."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import conditional_granger_ref as cref
import linear_dependence_ref as lref

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_group_sizes", "test_three_uneven_groups_string_labels", "test_pairwise_tier",
                       "test_invariance_on_device", "test_zero_and_nyquist_bins", "test_real_coefficients",
                       "test_torch_free_host_gives_the_same_values")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 16), (8, 8), (16, 17), (32, 32), (63, 65), (64, 64), (1, 127)]
NAMES = ("total", "instantaneous", "lagged")


def bounds(precision):
    return (1e-9, 1e-9) if precision == "dtype" else (1e-4, 1e-4)


def assert_close(got, ref, atol, rtol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN patterns differ"
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    print(f"ACCURACY {what}: worst error {err.max():.3e}, worst error / (atol + rtol |ref|) {(err / (atol + rtol * np.abs(ref[ok]))).max():.3e}")
    excess = err - (atol + rtol * np.abs(ref[ok]))
    assert excess.max() <= 0, f"{what}: worst excess {excess.max():.3e} (atol {atol}, rtol {rtol})"


def device(S, expectation_type="tapers"):
    import spectral_connectivity_amd as sc
    return sc.Connectivity(cref.coefficients_for(S), expectation_type=expectation_type)


@functools.lru_cache(maxsize=None)
def sized_case(sizes):
    """(two-sided spectra, permuted labels, reference (total, instantaneous, lagged, labels)) of a size pair, computed once."""
    na, nb = sizes
    C = na + nb
    S = lref.var_spectrum(C, C)
    labels = np.r_[np.zeros(na, int), np.ones(nb, int)][np.random.default_rng(C).permutation(C)]
    return S, labels, lref.dependence(S[:17], labels)


@functools.lru_cache(maxsize=None)
def labelled_case(C, seed, labels):
    S = lref.var_spectrum(C, seed)
    return S, lref.dependence(S[:17], None if labels is None else np.array(labels))


def check_identities(dep, what):
    off = ~np.isnan(dep.total)
    assert np.array_equal(np.isnan(dep.lagged), ~off) and np.array_equal(np.isnan(dep.instantaneous), ~off)
    assert dep.lagged[off].min() >= -1e-9, f"{what}: lagged part {dep.lagged[off].min():.3e}"
    gap = np.abs(dep.total[off] - (dep.instantaneous[off] + dep.lagged[off])) / (1.0 + np.abs(dep.total[off]))
    assert gap.max() <= 1e-12, f"{what}: total - (instantaneous + lagged) = {gap.max():.3e} (1 + |total|)"
    for v in (dep.total, dep.instantaneous, dep.lagged):
        assert np.array_equal(v, np.swapaxes(v, -1, -2), equal_nan=True), f"{what}: not symmetric"
        assert np.isnan(np.einsum("...ii->...i", v)).all(), f"{what}: diagonal"


@pytest.mark.parametrize("sizes", SIZES, ids=[f"{a}x{b}" for a, b in SIZES])
def test_group_sizes(sizes, _engine_precision):
    """Group sizes at every edge: single signals (the pairwise kernel), one signal against a group, odd sizes, 128 joint signals
    in three splits; labels permuted over the channels."""
    S, labels, ref = sized_case(sizes)
    dep = device(S).linear_dependence(labels)
    assert list(dep.labels) == [0, 1] and dep.total.dtype == np.float64 and dep.total.shape == (1, 1, 17, 2, 2)
    atol, rtol = bounds(_engine_precision)
    for name, want in zip(NAMES, ref):
        assert_close(getattr(dep, name).reshape(want.shape), want, atol, rtol, f"{_engine_precision} {sizes} {name}")
    check_identities(dep, str(sizes))
    assert ref[2][1:-1, 0, 1].max() > 1e-3


def test_three_uneven_groups_string_labels(_engine_precision):
    """Unsorted string labels come back sorted; groups of 1, 20 and 7 channels in one launch."""
    rng = np.random.default_rng(5)
    labels = tuple(np.array(["v1"] * 1 + ["pfc"] * 20 + ["lgn"] * 7)[rng.permutation(28)].tolist())
    S, ref = labelled_case(28, 5, labels)
    dep = device(S).linear_dependence(np.array(labels))
    assert list(dep.labels) == ["lgn", "pfc", "v1"] and list(ref[3]) == ["lgn", "pfc", "v1"]
    atol, rtol = bounds(_engine_precision)
    for name, want in zip(NAMES, ref):
        assert_close(getattr(dep, name).reshape(want.shape), want, atol, rtol, f"{_engine_precision} (1, 20, 7) {name}")
    check_identities(dep, "three groups")


@pytest.mark.parametrize("C", [7, 33])
def test_pairwise_tier(C, _engine_precision):
    """linear_dependence() and lagged_coherence() of single signals against the closed forms; 33: an odd count on the pad channel
    of the records, three tiles of the kernel."""
    S = lref.var_spectrum(C, 40 + C)
    c = device(S)
    dep = c.linear_dependence()
    rho2 = c.lagged_coherence()
    assert np.array_equal(dep.labels, np.arange(C)) and dep.total.shape == rho2.shape == (1, 1, 17, C, C)
    ct, ci, cl, cr = lref.pairwise_closed(S[:17])
    atol, rtol = bounds(_engine_precision)
    for name, want in zip(NAMES + ("lagged coherence",), (ct, ci, cl, cr)):
        got = rho2 if name == "lagged coherence" else getattr(dep, name)
        assert_close(got.reshape(want.shape), want, atol, rtol, f"{_engine_precision} pairwise {C} {name}")
    check_identities(dep, f"pairwise {C}")
    assert np.nanmin(rho2) >= 0.0 and np.nanmax(rho2) <= 1.0 and np.nanmax(rho2[..., 1:-1, :, :]) > 1e-3


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


def test_lagged_coherence_of_a_multitaper_estimate():
    """On a Multitaper estimate, float64 engine: lagged_coherence() = Im^2 / (1 - Re^2) of coherency()."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import options
    options.precision = "dtype"            # (the package default; the fixture puts the module's selection back afterwards)
    c = sc.Connectivity.from_multitaper(multitaper(lagged_series()))
    rho2 = c.lagged_coherence()
    coh = c.coherency()
    assert rho2.shape == coh.shape and rho2.dtype == np.float64
    off = ~np.eye(6, dtype=bool)
    np.testing.assert_allclose(rho2[..., off], coh.imag[..., off] ** 2 / (1 - coh.real[..., off] ** 2), rtol=1e-10, atol=1e-10)
    assert np.isnan(rho2[..., ~off]).all() and np.nanmax(rho2) > 0.1


def test_group_kernel_agrees_with_the_pairwise_kernel():
    """A labelling with one group of two signals sends every pair to the group kernel: its pair of single signals must equal the
    pairwise kernel's entry (both are float64 arithmetic on the same record, a 2 x 2 matrix of condition number < 100: 1e-12)."""
    S = lref.var_spectrum(4, 16)
    c = device(S)
    single = c.linear_dependence(np.arange(4))
    grouped = c.linear_dependence([0, 1, 2, 2])
    assert grouped.total.shape == (1, 1, 17, 3, 3)
    for name in NAMES:
        a, b = getattr(single, name)[..., 0, 1], getattr(grouped, name)[..., 0, 1]
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-12 * (1.0 + np.abs(a).max()), (name, np.abs(a - b).max())
    assert single.total[..., 0, 1].max() > 0.1 and single.lagged[..., 0, 1].max() > 0.1


def test_zero_and_nyquist_bins(_engine_precision):
    """Real series: the cross-spectrum is real at the zero and Nyquist bins, so the lagged part is 0 there."""
    import spectral_connectivity_amd as sc
    x = lagged_series(seed=9)
    labels = np.array([0, 0, 1, 1, 2, 2])
    c = sc.Connectivity.from_multitaper(multitaper(x, n_fft_samples=128))
    dep = c.linear_dependence(labels)
    assert dep.lagged.shape[-3] == 65
    tol = 1e-7 if _engine_precision == "dtype" else 1e-3
    off = ~np.eye(3, dtype=bool)
    edge = dep.lagged[..., [0, -1], :, :][..., off]
    assert np.isfinite(edge).all() and np.abs(edge).max() <= tol
    assert np.nanmax(dep.lagged[..., 1:-1, :, :]) > 0.05
    rho2 = c.lagged_coherence()[..., [0, -1], :, :][..., ~np.eye(6, dtype=bool)]
    assert np.isfinite(rho2).all() and np.abs(rho2).max() <= tol


def test_real_coefficients(_engine_precision):
    """Real Fourier coefficients (purely instantaneous mixing): the pairwise lagged coherence is exactly 0, the group F_lagged
    the difference of two factorisations of the same real matrix (<= 1e-10 in magnitude)."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(9)
    coef = rng.standard_normal((1, 1, 12, 16, 6)).astype(complex)
    c = sc.Connectivity(coef, expectation_type="tapers")
    rho2 = c.lagged_coherence()
    off = ~np.eye(6, dtype=bool)
    assert np.all(rho2[..., off] == 0.0)
    assert np.all(c.linear_dependence().lagged[..., off] == 0.0)
    dep = c.linear_dependence([0, 0, 1, 1, 2, 2])
    off3 = ~np.eye(3, dtype=bool)
    assert np.isfinite(dep.lagged[..., off3]).all() and np.abs(dep.lagged[..., off3]).max() <= 1e-10
    assert dep.total[..., off3].min() > 1e-3


def test_invariance_on_device(_engine_precision):
    """A real invertible mix of each group's time series leaves all three unchanged."""
    import spectral_connectivity_amd as sc
    x = lagged_series(seed=8)
    labels = np.array([0, 1, 0, 1, 2, 2])
    rng = np.random.default_rng(8)
    T = np.zeros((6, 6))
    for lab in range(3):
        idx = np.flatnonzero(labels == lab)
        T[np.ix_(idx, idx)] = np.eye(len(idx)) + 0.5 * rng.standard_normal((len(idx), len(idx)))
    a = sc.Connectivity.from_multitaper(multitaper(x)).linear_dependence(labels)
    b = sc.Connectivity.from_multitaper(multitaper(x @ T.T)).linear_dependence(labels)
    tol = 1e-8 if _engine_precision == "dtype" else 2e-3
    for name in NAMES:
        got, want = getattr(b, name), getattr(a, name)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max() <= tol * max(1.0, np.abs(want[ok]).max()), name
    assert np.nanmax(a.lagged) > 0.05


def test_errors():
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)
    coef = rng.standard_normal((1, 1, 8, 8, 6)) + 1j * rng.standard_normal((1, 1, 8, 8, 6))
    c = sc.Connectivity(coef, expectation_type="tapers")
    with pytest.raises(ValueError, match="at least two groups"):
        c.linear_dependence([3] * 6)
    with pytest.raises(ValueError, match="one label per signal"):
        c.linear_dependence([0, 1, 0, 1])
    big = rng.standard_normal((1, 1, 2, 4, 129)) + 1j * rng.standard_normal((1, 1, 2, 4, 129))
    with pytest.raises(ValueError, match="groups 'a' and 'b' have 129 signals together"):
        sc.Connectivity(big, expectation_type="tapers").linear_dependence(["a"] * 2 + ["b"] * 127)
    x = rng.standard_normal((512, 2, 3))
    with pytest.raises(ValueError, match="Connectivity class directly"):
        sc.multitaper_connectivity(x, 200.0, method="linear_dependence", time_halfbandwidth_product=2, time_window_duration=0.64)


def test_entry_point_refuses_a_pair_of_129_signals():
    """The entry point itself, groups of (2, 127) signals in device arrays: SC_EUNSUPPORTED with the pair size, from the sizes it
    reads back before any launch (the records are never touched)."""
    import torch
    from spectral_connectivity_amd import _lib, _stage_d, engine
    mem = engine.TorchMemory(torch.device("cuda", torch.cuda.current_device()))
    members, sizes, stride = _lib.member_table([np.arange(2), np.arange(2, 129)])
    assert stride == 128
    accum = torch.zeros((1, 2 * 45 * 256), dtype=torch.float64, device=mem.device)       # one record of 129 signals (9 x 9 tiles)
    with pytest.raises(_lib.HipEngineError, match=r"status -5.*129"):
        _stage_d.linear_dependence(mem, accum, 129, _lib.PLANE_CSM, 200, members, sizes, ("total",))


def test_labelled_interface_serves_lagged_coherence_by_name():
    import spectral_connectivity_amd as sc
    x = lagged_series(T=512, R=4, seed=4)
    kw = dict(time_halfbandwidth_product=2, time_window_duration=0.64)
    out = sc.multitaper_connectivity(x, 200.0, method="lagged_coherence", **kw)
    assert out.name == "lagged_coherence" and tuple(out.dims) == ("time", "frequency", "source", "target")
    m = sc.Multitaper(x, sampling_frequency=200.0, **kw)
    want = sc.Connectivity.from_multitaper(m).lagged_coherence()
    np.testing.assert_allclose(np.asarray(out.values), want, rtol=1e-12, atol=1e-14, equal_nan=True)
    assert np.nanmax(want) > 0.1


def test_rank_rule(caplog):
    """5 observations, groups of 2, 3 and 4 signals: the pairs (2, 4) and (3, 4) have more signals than observations -- NaN, not
    computed, one warning that counts them; the pair (2, 3) is computed."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(2)
    coef = rng.standard_normal((1, 1, 5, 16, 9)) + 1j * rng.standard_normal((1, 1, 5, 16, 9))
    labels = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2])
    c = sc.Connectivity(coef, expectation_type="tapers")
    with caplog.at_level(logging.WARNING):
        dep = c.linear_dependence(labels)
    msgs = [r.getMessage() for r in caplog.records if "linear dependence" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith("linear dependence: 2 group pairs have more signals together than the 5 observations")
    for v in dep[:3]:
        v = v.reshape(-1, 3, 3)
        assert np.isnan(v[:, 1, 2]).all() and np.isnan(v[:, 0, 2]).all() and np.isfinite(v[:, 0, 1]).all()
    assert dep.total.reshape(-1, 3, 3)[:, 0, 1].min() > 0.0 and dep.lagged.reshape(-1, 3, 3)[:, 0, 1].min() >= -1e-9


def test_all_zero_channel(caplog):
    """A channel whose coefficients are all zero has no power: the pairs of its group are NaN, one warning with their count."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(3)
    coef = rng.standard_normal((1, 1, 8, 16, 6)) + 1j * rng.standard_normal((1, 1, 8, 16, 6))
    coef[..., 4] = 0.0
    labels = np.array([0, 0, 1, 1, 2, 2])
    c = sc.Connectivity(coef, expectation_type="tapers")
    with caplog.at_level(logging.WARNING):
        dep = c.linear_dependence(labels)
    for v in dep[:3]:
        v = v.reshape(-1, 3, 3)
        assert np.isnan(v[:, 2, :]).all() and np.isnan(v[:, :, 2]).all() and np.isfinite(v[:, 0, 1]).all()
    msgs = [r.getMessage() for r in caplog.records if "linear dependence" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith(f"linear dependence: {2 * 9} (frequency, pair) problems")     # 2 pairs x 9 bins
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        rho2 = c.lagged_coherence().reshape(-1, 6, 6)
    assert np.isnan(rho2[:, 4, :]).all() and np.isnan(rho2[:, :, 4]).all() and np.isfinite(rho2[:, 0, 1]).all()
    msgs = [r.getMessage() for r in caplog.records if "linear dependence" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith(f"linear dependence: {5 * 9} (frequency, pair) problems")     # 5 pairs x 9 bins


def test_torch_free_host_gives_the_same_values(_engine_precision):
    S = lref.var_spectrum(9, 21)
    labels = np.array([2, 0, 1, 2, 0, 1, 1, 0, 2])
    c = device(S)
    dep = c.linear_dependence(labels)
    here = np.stack(dep[:3])
    pair = c.lagged_coherence()
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
dep = c.linear_dependence(np.array([2, 0, 1, 2, 0, 1, 1, 0, 2]))
assert type(dep).__name__ == "LinearDependence" and dep._fields == ("total", "instantaneous", "lagged", "labels")
assert list(dep.labels) == [0, 1, 2]
np.savez(sys.argv[4], groups=np.stack(dep[:3]), pair=c.lagged_coherence())
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sp, op = os.path.join(tmp, "S.npy"), os.path.join(tmp, "out.npz")
        np.save(sp, S)
        env = dict(os.environ, SC_HIP_HOST="numpy")
        out = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, sp, op], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "numpy host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        other = np.load(op)
        np.testing.assert_allclose(other["groups"], here, rtol=1e-12, atol=1e-14, equal_nan=True)
        np.testing.assert_allclose(other["pair"], pair, rtol=1e-12, atol=1e-14, equal_nan=True)


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU): the bins split over the ranks, the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29593",
                          os.path.join(ROOT, "tools", "check_sharded_dependence.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sharded linear dependence OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
