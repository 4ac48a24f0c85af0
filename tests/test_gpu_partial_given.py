"""Partial and multiple coherence GIVEN a chosen set of signals on the device (sc_partial_coherence_given_f64 through the
``given`` / ``signals`` keywords of Connectivity.partial_coherency / partial_coherence_magnitude / multiple_coherence_magnitude)
against the NumPy float64 reference of tests/partial_given_ref.py.

Exact spectra go in through the public API as uploaded Fourier coefficients whose taper average is S(f)
(conditional_granger_ref.coefficients_for), 17 bins a case.  Bounds: the project's own for these inputs, bounds() = 1e-9
absolute + relative on the float64 engine and 1e-4 on the float32 engines.  Every case asserts on the reference, before it
compares, that the unit-diagonal given block has a condition number <= 100 and that every residual share r_i is >= 0.1 -- better
conditioned than the full 128-signal inverse that passes the same bounds --, so a changed generator cannot loosen a case
unnoticed."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import conditional_granger_ref as cref
import partial_coherence_ref as pref
import partial_given_ref as gref
from test_gpu_imaginary_interaction import assert_close, bounds, var_spectrum
from test_gpu_partial_coherence import series_bound

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_exact_spectra", "test_sizes", "test_largest_kept_set_the_lds_admits", "test_beyond_the_lds_budget",
                       "test_all_the_others_given_equals_the_existing_methods", "test_without_keywords_nothing_changes",
                       "test_common_driver", "test_order_of_the_lists", "test_zero_and_nyquist_bins", "test_units",
                       "test_too_few_observations", "test_copy_of_a_given_signal", "test_duplicated_given_signal",
                       "test_torch_free_host_gives_the_same_values", "test_from_a_time_series")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FREQ = 17
NAMES = ("partial_coherency", "partial_coherence_magnitude", "multiple_coherence_magnitude")


@functools.lru_cache(maxsize=None)
def spectrum(n_signals, seed):
    S = var_spectrum(n_signals, seed)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def coefficients(n_signals, seed):
    coef = cref.coefficients_for(np.asarray(spectrum(n_signals, seed)))
    coef.setflags(write=False)
    return coef


@functools.lru_cache(maxsize=None)
def case(n_signals, a, m):
    """(kept: a sorted random subset, given: a random subset in random order, reference coherency [17, a, a], reference multiple
    coherence [17, a]) on spectrum(n_signals, n_signals), computed once and shared read-only.  The conditioning of the case is
    asserted here, on the reference."""
    S = spectrum(n_signals, n_signals)[:N_FREQ]
    perm = np.random.default_rng(1000 * n_signals + a).permutation(n_signals)
    given, kept = perm[:m].copy(), np.sort(perm[m:m + a])
    cond, r_min = gref.conditioning(S, kept, given)
    assert cond <= 100.0 and r_min >= 0.1, f"({n_signals}, {a}, {m}): cond {cond:.1f}, min r {r_min:.3f}"
    gamma, multiple = gref.schur(S, kept, given)
    for arr in (kept, given, gamma, multiple):
        arr.setflags(write=False)
    return kept, given, gamma, multiple


def device(n_signals, seed, expectation_type="tapers", scale=None):
    import spectral_connectivity_amd as sc
    coef = coefficients(n_signals, seed)
    if scale is not None:
        coef = coef * scale
    return sc.Connectivity(coef, expectation_type=expectation_type)


def all_three(c, given, signals=None):
    return tuple(getattr(c, name)(given=given, signals=signals) for name in NAMES)


def check_against(got, gamma, multiple, precision, what):
    coherency, magnitude, mult = got
    atol, rtol = bounds(precision)
    assert coherency.dtype == np.complex128 and magnitude.dtype == np.float64 and mult.dtype == np.float64
    if gamma.shape[-1] == 1:                                     # one kept signal: no pair, only the NaN diagonal
        assert coherency.size == magnitude.size == gamma.size and np.isnan(coherency).all() and np.isnan(magnitude).all()
    else:
        assert_close(coherency.reshape(gamma.shape), gamma, atol, rtol, f"{what}: partial coherency")
        assert_close(magnitude.reshape(gamma.shape), np.abs(gamma), atol, rtol, f"{what}: partial coherence magnitude")
    assert_close(mult.reshape(multiple.shape), multiple, atol, rtol, f"{what}: multiple coherence magnitude")


def check_symmetry(coherency, magnitude, mult):
    a = coherency.shape[-1]
    diag = np.eye(a, dtype=bool)
    assert np.isnan(coherency[..., diag]).all() and np.isnan(magnitude[..., diag]).all()
    assert np.isfinite(coherency[..., ~diag]).all() and np.isfinite(mult).all()
    # Hermitian exactly: the kernel writes one value and its conjugate
    assert np.array_equal(coherency[..., ~diag], np.conj(np.swapaxes(coherency, -1, -2))[..., ~diag])
    assert np.array_equal(magnitude[..., ~diag], np.swapaxes(magnitude, -1, -2)[..., ~diag])
    if a > 1:
        assert magnitude[..., ~diag].max() <= 1.0 + 1e-12
    assert 0.0 <= mult.min() and mult.max() <= 1.0


@pytest.mark.parametrize("expectation_type", ["tapers", "trials_tapers"])
def test_exact_spectra(expectation_type, _engine_precision):
    n, a, m = 7, 3, 4
    kept, given, gamma, multiple = case(n, a, m)
    coherency, magnitude, mult = got = all_three(device(n, n, expectation_type), given, kept)
    lead = (1, 1) if expectation_type == "tapers" else (1,)
    assert coherency.shape == magnitude.shape == lead + (N_FREQ, a, a) and mult.shape == lead + (N_FREQ, a)
    check_symmetry(*got)
    check_against(got, gamma, multiple, _engine_precision, expectation_type)
    off = ~np.eye(a, dtype=bool)
    assert np.abs(gamma[1:-1][..., off].imag).max() > 0.01       # (the phase is compared, not only the magnitude)


# (n_signals, kept, given): the smallest; both sides of the 64 KB of LDS a launch gets without asking; one kept signal (no pair);
# one given signal; 16 / 17 on either side (the record tile edge); 128 given out of more than 128 signals; the wide arrays -- 300
# kept signals walk 38 x 38 output tiles --; a = 255, 256, 257 around the stride of the 256 threads
SIZES = [(7, 3, 4), (128, 2, 126), (128, 64, 64), (128, 1, 127), (40, 39, 1), (33, 16, 17), (34, 17, 16), (140, 12, 128),
         (306, 300, 6), (257, 255, 2), (258, 256, 2), (259, 257, 2)]


@pytest.mark.parametrize("n, a, m", SIZES)
def test_sizes(n, a, m, _engine_precision):
    kept, given, gamma, multiple = case(n, a, m)
    got = all_three(device(n, n), given, kept)
    assert got[0].shape == (1, 1, N_FREQ, a, a) and got[2].shape == (1, 1, N_FREQ, a)
    check_symmetry(*got)
    check_against(got, gamma, multiple, _engine_precision, f"({n}, {a}, {m})")


@pytest.mark.parametrize("m", [128, 17])
def test_largest_kept_set_the_lds_admits(m, _engine_precision):
    """The largest kept set the library's own LDS query admits for m given signals (14 at m = 128, 559 at m = 17; at most what a
    record holds), and ValueError with the numbers for one kept signal more."""
    from spectral_connectivity_amd import _lib
    lib = _lib.load()
    limit, max_kept = lib.sc_partial_given_lds_limit(), lib.sc_partial_given_max_kept()
    assert limit == 160 * 1024
    a = max(k for k in range(1, max_kept + 1) if lib.sc_partial_given_lds_bytes(k, m) <= limit)
    a = min(a, _lib.PLANES_FORMAT_MAX_CHANNELS - m - 1)
    assert a == {128: 14, 17: 559}[m]
    n = a + 1 + m
    kept, given, gamma, multiple = case(n, a, m)
    c = device(n, n)
    got = all_three(c, given, kept)
    check_symmetry(*got)
    check_against(got, gamma, multiple, _engine_precision, f"({n}, {a}, {m})")
    one_more = np.setdiff1d(np.arange(n), given)
    assert len(one_more) == a + 1
    for name in NAMES:
        with pytest.raises(ValueError, match=f"{a + 1} kept signals given {m}"):
            getattr(c, name)(given=given, signals=one_more)


def test_beyond_the_lds_budget(_engine_precision):
    """192 kept signals given 128: W alone is 128 x 192 complex = 384 KB, and sc_partial_given_lds_bytes(192, 128) = 529 424 bytes
    against the 160 KB of a compute unit -- the limit that test_largest_kept_set_the_lds_admits pins at 14 kept signals for 128
    given.  The request is refused with the numbers, before any device work."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import _lib
    assert _lib.load().sc_partial_given_lds_bytes(192, 128) == 529424
    rng = np.random.default_rng(1)
    c = sc.Connectivity(rng.standard_normal((1, 1, 2, 4, 320)) + 1j * rng.standard_normal((1, 1, 2, 4, 320)), expectation_type="tapers")
    perm = rng.permutation(320)
    for name in NAMES:
        with pytest.raises(ValueError, match="192 kept signals given 128 needs 529424 bytes"):
            getattr(c, name)(given=perm[:128], signals=np.sort(perm[128:]))
        with pytest.raises(ValueError, match="at most 128 given"):
            getattr(c, name)(given=perm[:129], signals=perm[129:131])


@pytest.mark.parametrize("n", [7, 128])
def test_all_the_others_given_equals_the_existing_methods(n, _engine_precision):
    """signals = [i, j] given all the others is partial_coherency()[..., i, j]; signals = [i] given all the others is
    multiple_coherence_magnitude()[..., i]."""
    c = device(n, n)
    atol, rtol = bounds(_engine_precision)
    full, full_mag, full_mult = c.partial_coherency(), c.partial_coherence_magnitude(), c.multiple_coherence_magnitude()
    for i, j in ((0, 1), (n - 1, 2), (3, n - 2)):
        others = [k for k in range(n) if k not in (i, j)]
        coherency, magnitude, _ = all_three(c, others, [i, j])
        assert coherency.shape == (1, 1, N_FREQ, 2, 2)
        assert_close(coherency[..., 0, 1], full[..., i, j], atol, rtol, f"pair ({i}, {j}) given the others")
        assert_close(coherency[..., 1, 0], full[..., j, i], atol, rtol, f"pair ({j}, {i}) given the others")
        assert_close(magnitude[..., 0, 1], full_mag[..., i, j], atol, rtol, f"|pair ({i}, {j})| given the others")
    for i in (0, n // 2, n - 1):
        mult = c.multiple_coherence_magnitude(given=[k for k in range(n) if k != i], signals=[i])
        assert mult.shape == (1, 1, N_FREQ, 1)
        assert_close(mult[..., 0], full_mult[..., i], atol, rtol, f"signal {i} given the others")
        one = c.partial_coherency(given=[k for k in range(n) if k != i], signals=[i])
        assert one.shape == (1, 1, N_FREQ, 1, 1) and np.isnan(one).all()


def test_without_keywords_nothing_changes(_engine_precision):
    c = device(7, 7)
    for name in NAMES:
        plain, explicit = getattr(c, name)(), getattr(c, name)(given=None, signals=None)
        assert plain.dtype == explicit.dtype and plain.shape == explicit.shape
        assert plain.tobytes() == explicit.tobytes()
        with pytest.raises(ValueError, match="needs `given`"):
            getattr(c, name)(signals=[0, 1])


def test_common_driver(_engine_precision):
    """x1 and x2 are delayed noisy copies of x3: coherent, and not at all once x3 is given; the driver explains sigma / (sigma +
    s_k) of the power of copy k."""
    import spectral_connectivity_amd as sc
    S, sigma, noise = pref.common_driver_spectrum()
    c = sc.Connectivity(cref.coefficients_for(S), expectation_type="tapers")
    coherency, magnitude, mult = all_three(c, [2], [0, 1])
    atol, rtol = bounds(_engine_precision)
    assert coherency.shape == (1, 1, N_FREQ, 2, 2)
    assert np.abs(coherency[..., 0, 1]).max() <= atol and magnitude[..., 0, 1].max() <= atol
    assert c.coherence_magnitude()[..., 0, 1].min() > 0.3
    for k in (0, 1):
        closed = np.sqrt(sigma / (sigma + noise[k]))[:N_FREQ]
        assert_close(mult.reshape(N_FREQ, 2)[:, k], closed, atol, rtol, f"R_{k + 1} against its closed form")


def test_order_of_the_lists(_engine_precision):
    n = 9
    c = device(n, 21)
    given = [7, 0, 4]
    sorted_ = all_three(c, given, [1, 3, 5])
    permuted = all_three(c, given, [5, 1, 3])
    p = [2, 0, 1]                                            # [5, 1, 3] out of [1, 3, 5]
    atol, rtol = bounds(_engine_precision)
    assert_close(permuted[0], sorted_[0][..., p, :][..., :, p], atol, rtol, "signals permuted: coherency")
    assert_close(permuted[1], sorted_[1][..., p, :][..., :, p], atol, rtol, "signals permuted: magnitude")
    assert np.array_equal(permuted[2], sorted_[2][..., p])
    assert np.abs(sorted_[0][..., 0, 1] - sorted_[0][..., 0, 2])[..., 1:-1].min() > 1e-3      # (a permutation is visible)
    for x, y, what in zip(all_three(c, [4, 7, 0], [1, 3, 5]), sorted_, NAMES):
        assert_close(x, y, atol, rtol, f"given permuted: {what}")
    default = all_three(c, given)
    assert default[0].shape == (1, 1, N_FREQ, 6, 6)
    explicit = all_three(c, given, [1, 2, 3, 5, 6, 8])
    for x, y in zip(default, explicit):
        assert np.array_equal(x, y, equal_nan=True)


def test_zero_and_nyquist_bins(_engine_precision):
    """The spectrum of a real process is real at the zero and the Nyquist bin, and so is the partial coherency there."""
    n, kept, given = 5, [0, 2, 4], [3, 1]
    S = spectrum(n, 9)
    assert np.abs(S[[0, 16]].imag).max() <= 1e-15
    gamma, multiple = gref.schur(S[:N_FREQ], kept, given)
    coherency, _, _ = got = all_three(device(n, 9), given, kept)
    check_against(got, gamma, multiple, _engine_precision, "5 signals")
    off = ~np.eye(3, dtype=bool)
    atol, _ = bounds(_engine_precision)
    at_edge = coherency.reshape(gamma.shape)[[0, N_FREQ - 1]][:, off]
    assert np.isfinite(at_edge).all() and np.abs(at_edge.imag).max() <= atol
    assert np.abs(at_edge.real).max() > 0.02
    assert np.abs(coherency.reshape(gamma.shape)[1:-1][:, off].imag).max() > 0.01


def test_units(_engine_precision):
    """Channel k in units 10^(3 k / C - 1.5) times larger: three decades across the array, and the same results."""
    n, kept, given = 7, [6, 0, 3, 2], [5, 1]
    gamma, multiple = gref.schur(spectrum(n, 11)[:N_FREQ], kept, given)
    units = 10.0 ** (3.0 * np.arange(n) / n - 1.5)
    plain, scaled = all_three(device(n, 11), given, kept), all_three(device(n, 11, scale=units), given, kept)
    check_against(scaled, gamma, multiple, _engine_precision, "scaled channels")
    atol, rtol = bounds(_engine_precision)
    for x, y, what in zip(scaled, plain, NAMES):
        assert_close(x, y, atol, rtol, f"scaled against plain channels: {what}")


def test_too_few_observations(caplog, _engine_precision):
    """3 observations and 3 given signals: the given block spans the observations and nothing is left -- NaN of the right
    shape, one warning a method, no launch."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(2)
    coef = rng.standard_normal((1, 1, 3, 16, 6)) + 1j * rng.standard_normal((1, 1, 3, 16, 6))
    c = sc.Connectivity(coef, expectation_type="tapers")
    for name, shape, dtype in ((NAMES[0], (1, 1, 9, 3, 3), np.complex128), (NAMES[1], (1, 1, 9, 3, 3), np.float64),
                               (NAMES[2], (1, 1, 9, 3), np.float64)):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            out = getattr(c, name)(given=[0, 2, 4])
        assert out.shape == shape and out.dtype == dtype and np.isnan(out).all()
        msgs = [r.getMessage() for r in caplog.records if "partial coherence" in r.getMessage()]
        assert len(msgs) == 1 and "3 given signals from 3 observations" in msgs[0]


def singular_coefficients(copy_to, copy_from):
    rng = np.random.default_rng(3)
    coef = rng.standard_normal((1, 1, 8, 16, 6)) + 1j * rng.standard_normal((1, 1, 8, 16, 6))
    coef[..., copy_to] = coef[..., copy_from]
    return coef


def test_copy_of_a_given_signal(caplog, _engine_precision):
    """8 observations of 6 signals, signal 4 a copy of the given signal 1: nothing is left of it -- its row and column are NaN and
    the given signals explain all of it; every other entry is as the reference has it."""
    import spectral_connectivity_amd as sc
    coef = singular_coefficients(4, 1)
    c = sc.Connectivity(coef, expectation_type="tapers")
    X = np.asarray(coef[0, 0], dtype=np.complex128 if _engine_precision == "dtype" else np.complex64).astype(np.complex128)
    S = np.einsum("kfi,kfj->fij", X, np.conj(X))[:9] / 8.0
    kept, given = [0, 3, 4, 5], [1, 2]
    with np.errstate(all="ignore"):
        gamma, multiple = gref.schur(S, kept, given)
    gamma[:, 2, :] = np.nan
    gamma[:, :, 2] = np.nan
    multiple[:, 2] = 1.0
    for name, ref in zip(NAMES, (gamma, np.abs(gamma), multiple)):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            out = getattr(c, name)(given=given)
        assert out.shape == (1, 1) + ref.shape
        assert_close(out[0, 0], ref, *bounds(_engine_precision), name)
        if name == NAMES[2]:
            assert np.all(out[0, 0, :, 2] == 1.0)
        msgs = [r.getMessage() for r in caplog.records if "partial coherence" in r.getMessage()]
        assert len(msgs) == 1 and msgs[0].startswith("partial coherence: 9 (bin, signal) cases"), msgs


def test_duplicated_given_signal(caplog, _engine_precision):
    """Two identical given signals: their block has no Cholesky factor in any bin -- NaN everywhere, one warning with the count."""
    import spectral_connectivity_amd as sc
    c = sc.Connectivity(singular_coefficients(4, 1), expectation_type="tapers")
    for name in NAMES:
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            out = getattr(c, name)(given=[1, 4])
        assert out.shape[:3] == (1, 1, 9) and out.shape[3] == 4 and np.isnan(out).all()
        msgs = [r.getMessage() for r in caplog.records if "partial coherence" in r.getMessage()]
        assert len(msgs) == 1 and msgs[0].startswith("partial coherence: 9 matrices of the given signals have no inverse"), msgs


def test_torch_free_host_gives_the_same_values(_engine_precision):
    n, given, signals = 9, [7, 0, 4], [5, 1, 3, 8]
    here = all_three(device(n, 21), given, signals)
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
kw = dict(given=[7, 0, 4], signals=[5, 1, 3, 8])
np.savez(sys.argv[4], coherency=c.partial_coherency(**kw), magnitude=c.partial_coherence_magnitude(**kw),
         multiple=c.multiple_coherence_magnitude(**kw))
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sp, op = os.path.join(tmp, "S.npy"), os.path.join(tmp, "out.npz")
        np.save(sp, spectrum(n, 21))
        env = dict(os.environ, SC_HIP_HOST="numpy")
        out = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, sp, op], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "numpy host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        other = np.load(op)
        for x, name in zip(here, ("coherency", "magnitude", "multiple")):
            assert other[name].dtype == x.dtype and other[name].shape == x.shape
            np.testing.assert_allclose(other[name], x, rtol=1e-12, atol=1e-14, equal_nan=True)


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU): the bins split over the ranks, the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29583",
                          os.path.join(ROOT, "tools", "check_sharded_partial_given.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sharded partial coherence given a set OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_labelled_interface_returns_the_kept_coordinates():
    """multitaper_connectivity(method=..., connectivity_kwargs={"given": ...}): source / target are the kept signals, the values
    the method's own."""
    import spectral_connectivity_amd as sc
    x = np.random.default_rng(4).standard_normal((512, 8, 4))
    x[:, :, 1] += 0.5 * x[:, :, 0]
    x[:, :, 2] += 0.5 * x[:, :, 0]
    kw = dict(time_halfbandwidth_product=2, time_window_duration=0.64)
    c = sc.Connectivity.from_multitaper(sc.Multitaper(x, sampling_frequency=200.0, **kw))
    out = sc.multitaper_connectivity(x, 200.0, method="partial_coherence_magnitude", connectivity_kwargs={"given": [0]}, **kw)
    assert tuple(out.dims) == ("time", "frequency", "source", "target")
    # (np.asarray: an xarray coordinate or the plain array of the vendored labelled arrays)
    assert list(np.asarray(out.coords["source"])) == ["1", "2", "3"] and list(np.asarray(out.coords["target"])) == ["1", "2", "3"]
    np.testing.assert_allclose(np.asarray(out.values), c.partial_coherence_magnitude(given=[0]), rtol=1e-12, atol=1e-14,
                               equal_nan=True)
    out = sc.multitaper_connectivity(x, 200.0, method="multiple_coherence_magnitude", signal_names=["a", "b", "c", "d"],
                                     connectivity_kwargs={"given": [0], "signals": [3, 1]}, **kw)
    assert tuple(out.dims) == ("time", "frequency", "source") and list(np.asarray(out.coords["source"])) == ["d", "b"]
    np.testing.assert_allclose(np.asarray(out.values), c.multiple_coherence_magnitude(given=[0], signals=[3, 1]), rtol=1e-12,
                               atol=1e-14)


def test_from_a_time_series(request, _engine_precision):
    """The data of test_gpu_partial_coherence.test_from_a_time_series (6 signals, 72 observations per window), given = [0, 5],
    against the Schur form on the float64 cross-spectra of the object's own coefficients.  float32 engines: series_bound(), the
    bound measured there for the full inverse of the same spectra -- an upper bound here, the given block being a principal
    submatrix of that scaled matrix (condition number <= 138, asserted)."""
    import spectral_connectivity_amd as sc
    engine = request.node.callspec.params["_engine_precision"]
    rng = np.random.default_rng(10)
    T, R, C, fs = 512, 24, 6, 200.0
    t = np.arange(T) / fs
    x = rng.standard_normal((T, R, C))
    x += np.linspace(0.5, 1.5, C)[None, None, :] * np.sin(2 * np.pi * 40.0 * t[:, None] + rng.uniform(0, 2 * np.pi, R)[None, :])[:, :, None]
    m = sc.Multitaper(x, sampling_frequency=fs, time_halfbandwidth_product=2, n_time_samples_per_window=128)
    c = sc.Connectivity.from_multitaper(m)
    given, kept = [0, 5], [1, 2, 3, 4]
    got = all_three(c, given)
    X = np.asarray(c.fourier_coefficients, dtype=np.complex128)          # [W, R, K, N, C]
    assert X.shape == (4, R, 3, 128, C) and c.n_observations == 72
    S = np.einsum("wrkfi,wrkfj->wfij", X, np.conj(X))[:, :65] / 72.0
    gamma, multiple = gref.schur(S, kept, given)
    cond, r_min = gref.conditioning(S, kept, given)
    d = np.einsum("wfii->wfi", S).real
    cond_full = np.linalg.cond(S / np.sqrt(d[..., :, None] * d[..., None, :])).max()
    assert cond <= cond_full <= 138.2 and r_min > 0.0
    assert got[0].shape == (4, 65, 4, 4) and got[1].shape == (4, 65, 4, 4) and got[2].shape == (4, 65, 4)
    off = ~np.eye(4, dtype=bool)
    worst = max(np.abs(got[0][..., off] - gamma[..., off]).max(), np.abs(got[1][..., off] - np.abs(gamma[..., off])).max(),
                np.abs(got[2] - multiple).max())
    print(f"\npartial coherence given [0, 5] from a time series, {engine}: worst |got - ref| = {worst:.3e}, "
          f"cond(given block) = {cond:.2f}, min r = {r_min:.3f}, cond(S') = {cond_full:.1f}")
    assert np.isnan(got[0][..., ~off]).all() and np.isnan(got[1][..., ~off]).all()
    assert worst <= series_bound(engine)
    assert np.abs(gamma[..., off]).max() > 0.1
