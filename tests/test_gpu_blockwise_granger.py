"""Blockwise spectral Granger prediction on the device (sc_blockwise.hip through
Connectivity.blockwise_spectral_granger_prediction) against the NumPy float64 reference of tests/blockwise_granger_ref.py.

Exact spectra go in through the public API as uploaded Fourier coefficients [1, 1, K = C, N, C] whose taper average is S(f)
(conditional_granger_ref.coefficients_for).  Large blocks are built with blockwise_granger_ref.embed: a small VAR core, independent
AR(1) signals and mixing inside each block, which leave the measure equal to the core's -- so the reference stays small while
the device factors the whole pair.  Bounds as tests/test_gpu_conditional_granger.py: 1e-6 absolute + relative on the float64
engine (two Wilson iterations at the same 1e-8 tolerance), 1e-4 on the float32 engines (float32 records, values that are logs of
ratios of Schur complements of the spectrum).  An entry that is NaN on one side only is allowed where the finite side is below
the absolute bound."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import blockwise_granger_ref as bref
import chunked_calls
import conditional_granger_ref as cref
from conftest import granger_close

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_two_blocks", "test_three_uneven_blocks_string_labels", "test_four_blocks_of_eight",
                       "test_large_pairs", "test_more_than_512_signals", "test_singletons_equal_pairwise_on_estimated_spectra",
                       "test_invariance_on_device", "test_torch_free_host_gives_the_same_values", "test_block_pairs_in_chunks",
                       "test_block_pairs_in_chunks_on_the_torch_free_host")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_var(C, seed, scale=0.35):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((1, C, C)) * (rng.random((1, C, C)) < min(0.5, 6.0 / C))
    A *= scale / max(np.abs(np.linalg.eigvals(A[0])).max(), 1e-3)
    L = np.eye(C) + 0.2 * np.tril(rng.standard_normal((C, C)), -1)
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
    return sc.Connectivity(cref.coefficients_for(S), expectation_type=expectation_type)


def squeeze(out):
    return out.reshape(out.shape[-3:])


@pytest.mark.parametrize("expectation_type", ["tapers", "trials_tapers"])
def test_two_blocks(expectation_type, _engine_precision):
    A, sigma = random_var(5, 1)
    S = cref.var_spectrum(A, sigma, 64)
    labels = [0, 1, 1, 0, 1]
    c = device(S, expectation_type)
    values, labs = c.blockwise_spectral_granger_prediction(labels)
    assert values.dtype == np.float64 and list(labs) == [0, 1]
    kept = (1, 1) if expectation_type == "tapers" else (1,)
    assert values.shape == kept + (33, 2, 2)
    assert c._last_wilson["status"].shape == (1, 1) and (c._last_wilson["status"] == 1).all()
    got = squeeze(values)
    assert np.isnan(got[:, [0, 1], [0, 1]]).all()
    ref, _ = bref.blockwise_granger(S, labels)
    assert_close(got, ref, *bounds(_engine_precision), what="3 + 2")
    assert np.isfinite(got[:, 0, 1]).all() and np.isfinite(got[:, 1, 0]).all()


def test_three_uneven_blocks_string_labels(_engine_precision):
    A, sigma = random_var(12, 2)
    S = cref.var_spectrum(A, sigma, 32)
    labels = np.array(["v1", "pfc", "pfc", "lgn", "pfc", "lgn", "lgn", "pfc", "lgn", "lgn", "lgn", "lgn"])   # 1, 4, 7
    values, labs = device(S).blockwise_spectral_granger_prediction(group_labels=labels)
    assert list(labs) == ["lgn", "pfc", "v1"]
    ref, _ = bref.blockwise_granger(S, labels)
    assert_close(squeeze(values), ref, *bounds(_engine_precision), what="1, 4, 7")


def test_four_blocks_of_eight(_engine_precision):
    A, sigma = random_var(32, 3)
    S = cref.var_spectrum(A, sigma, 32)
    labels = np.arange(32) % 4
    c = device(S)
    values, _ = c.blockwise_spectral_granger_prediction(labels)
    assert c._last_wilson["status"].shape == (6, 1)
    ref, _ = bref.blockwise_granger(S, labels)
    assert_close(squeeze(values), ref, *bounds(_engine_precision), what="4 x 8")


@pytest.mark.parametrize("sizes", [(31, 33), (1, 64), (64, 64), (65, 64), (128, 129)])
def test_large_pairs(sizes, _engine_precision):
    """m = 64 / 65 / 128 / 129 / 257: the MVAR kernels' boundaries (64, 128) and the epilogue's LDS / in-place boundary
    (blocks of 64 / 65 signals), n_a from 1 to 128."""
    A = np.array([[[0.4, 0.3, 0.0], [0.2, 0.3, 0.1], [0.0, 0.4, -0.3]]])          # coupled both ways: 0 <-> (1, 2)
    sigma = np.array([[1.0, 0.2, 0.0], [0.2, 1.0, 0.1], [0.0, 0.1, 1.0]])
    core = cref.var_spectrum(A, sigma, 64)          # (64 bins: the embedding is exact to 1e-8 -- 3e-5 on 32 for this VAR)
    core_labels = [0, 1, 1]
    S, labels = bref.embed(core, core_labels, sizes, seed=sum(sizes))
    values, _ = device(S).blockwise_spectral_granger_prediction(labels)
    ref, _ = bref.blockwise_granger(core, core_labels)
    assert np.isfinite(ref[:, 0, 1]).all() and np.isfinite(ref[:, 1, 0]).all()
    assert_close(squeeze(values), ref, *bounds(_engine_precision), what=f"blocks {sizes}")


def test_more_than_512_signals(_engine_precision):
    """600 signals in three blocks of 200: every pair has 400 signals, within the factorisation's 512, though the whole is not."""
    A, sigma = random_var(6, 31)
    core = cref.var_spectrum(A, sigma, 32)
    core_labels = [0, 1, 2, 0, 1, 2]
    S, labels = bref.embed(core, core_labels, (200, 200, 200), seed=600)
    c = device(S)
    values, labs = c.blockwise_spectral_granger_prediction(labels)
    assert values.shape == (1, 1, 17, 3, 3) and c._last_wilson["status"].shape == (3, 1)
    ref, _ = bref.blockwise_granger(core, core_labels)
    assert_close(squeeze(values), ref, *bounds(_engine_precision), what="3 x 200")


def test_singletons_equal_pairwise_on_estimated_spectra(_engine_precision):
    """Estimated spectra, every signal its own block: the pairwise measure, NaN pattern included (64-sample windows on 512
    bins, as the conditional measure's two-signal test)."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(7)
    T, R, C = 1024, 4, 4
    x = rng.standard_normal((T, R, C))
    for t in range(2, T):
        x[t, :, 0] += 0.55 * x[t - 1, :, 0] - 0.4 * x[t - 2, :, 0]
        x[t, :, 1] += 0.5 * x[t - 1, :, 1] + 0.45 * x[t - 1, :, 0]
        x[t, :, 3] += 0.3 * x[t - 1, :, 2] - 0.3 * x[t - 1, :, 3]
    m = sc.Multitaper(x, sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=64,
                      n_time_samples_per_step=64, n_fft_samples=512)
    c = sc.Connectivity.from_multitaper(m)
    values, labs = c.blockwise_spectral_granger_prediction(np.arange(C))
    assert c._last_wilson["status"].shape == (6, values.shape[0])
    pair = c.pairwise_spectral_granger_prediction()
    granger_close(values, pair, 2e-5, what="singleton blocks vs pairwise")
    assert np.nanmax(values[..., 1, 0]) > 0.1


def test_invariance_on_device(_engine_precision):
    """S and T S T^H, T = blockdiag(A_a, A_b) invertible: the same values (Geweke's invariance; a wrong Sigma~ or ordering
    breaks it)."""
    A, sigma = random_var(5, 5)
    S = cref.var_spectrum(A, sigma, 64)
    labels = np.array([1, 0, 1, 0, 1])
    rng = np.random.default_rng(8)
    T = np.zeros((5, 5))
    for lab in (0, 1):
        idx = np.flatnonzero(labels == lab)
        T[np.ix_(idx, idx)] = np.eye(len(idx)) + 0.5 * rng.standard_normal((len(idx), len(idx)))
    got = squeeze(device(S).blockwise_spectral_granger_prediction(labels)[0])
    mixed = squeeze(device(T @ S @ T.T).blockwise_spectral_granger_prediction(labels)[0])
    atol, rtol = bounds(_engine_precision)
    assert_close(mixed, got, atol, rtol, what="invariance")


def test_errors():
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)
    coef = rng.standard_normal((1, 1, 8, 8, 6)) + 1j * rng.standard_normal((1, 1, 8, 8, 6))
    c = sc.Connectivity(coef, expectation_type="tapers")
    with pytest.raises(TypeError):
        c.blockwise_spectral_granger_prediction()
    with pytest.raises(TypeError):
        c.blockwise_spectral_granger_prediction([0, 0, 0, 1, 1, 1], pairs=None)
    with pytest.raises(ValueError, match="at least two groups"):
        c.blockwise_spectral_granger_prediction([3] * 6)
    with pytest.raises(ValueError, match="one label per signal"):
        c.blockwise_spectral_granger_prediction([0, 1, 0, 1])
    big = np.zeros((1, 1, 1, 4, 520), dtype=complex)
    big[..., :] = 1.0
    with pytest.raises(ValueError, match="groups 'a' and 'b' have 520 signals"):
        sc.Connectivity(big, expectation_type="tapers").blockwise_spectral_granger_prediction(["a"] * 260 + ["b"] * 260)
    x = rng.standard_normal((512, 2, 3))
    with pytest.raises(ValueError, match="Connectivity class directly"):
        sc.multitaper_connectivity(x, 200.0, method="blockwise_spectral_granger_prediction", time_halfbandwidth_product=2,
                                   time_window_duration=0.64)


def test_rank_deficient_block(caplog):
    """Blocks of 1, 2 and 6 signals with 4 observations: the pairs with the 6-signal block have rank-deficient spectra -- NaN,
    one warning -- and the 1 + 2 pair is computed."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(2)
    coef = rng.standard_normal((1, 1, 4, 16, 9)) + 1j * rng.standard_normal((1, 1, 4, 16, 9))
    coef[..., 1] += 0.8 * np.roll(coef[..., 0], 1, axis=-1)
    labels = np.array([0, 1, 1, 2, 2, 2, 2, 2, 2])
    with caplog.at_level(logging.WARNING):
        values, _ = sc.Connectivity(coef, expectation_type="tapers").blockwise_spectral_granger_prediction(labels)
    got = squeeze(values)
    assert np.isnan(got[:, 2, :]).all() and np.isnan(got[:, :, 2]).all()
    assert np.isfinite(got[:, 0, 1]).any() or np.isfinite(got[:, 1, 0]).any()
    msgs = [r.getMessage() for r in caplog.records if "rank-deficient" in r.getMessage()]
    assert len(msgs) == 1 and msgs[0].startswith("blockwise Granger: 2 group pairs")


def test_torch_free_host_gives_the_same_values(_engine_precision):
    A, sigma = random_var(7, 21)
    S = cref.var_spectrum(A, sigma, 32)
    labels = np.array([2, 0, 1, 2, 0, 1, 1])
    got, _ = device(S).blockwise_spectral_granger_prediction(labels)
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
values, labels = c.blockwise_spectral_granger_prediction(np.array([2, 0, 1, 2, 0, 1, 1]))
np.save(sys.argv[4], values)
assert list(labels) == [0, 1, 2] and c._last_wilson["status"].shape == (3, 1)
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
    np.testing.assert_allclose(other, got, rtol=1e-9, atol=1e-12, equal_nan=True)


CHUNK_LABELS = np.array([0, 0, 1, 1, 2, 2, 3])          # groups of 2, 2, 2, 1: three pairs of m = 4 and three of m = 3


def chunked_and_whole(S):
    """The measure of ONE object with the default workspace bound and with the bound lowered to two block pairs per call, on
    whichever host the process runs: the two results, the statuses of the chunked run and (pairs, m) of each
    sc_blockwise_granger_f64 call it made.  The workspace of a pair grows with m, and no single bound gives two pairs per call at
    both m = 3 and m = 4 (at 32 bins the queries are 50944 / 73984 bytes for two / three pairs of m = 3, 86784 for two of m = 4),
    so _lib.CONDITIONAL_WORK_BYTES -- read when a batch is cut -- is lowered per batch, to the library's own query for two
    pairs of that batch's m."""
    from spectral_connectivity_amd import _lib
    c = device(S)
    whole, _ = c.blockwise_spectral_granger_prediction(CHUNK_LABELS)
    lib, real_chunk = _lib._handle(), _lib.blockwise_chunk

    def two_per_call(n_groups, n_pairs, workspace_bytes, cap=None):
        _lib.CONDITIONAL_WORK_BYTES = workspace_bytes(2)
        return real_chunk(n_groups, n_pairs, workspace_bytes, cap)

    with chunked_calls.replaced(_lib, "CONDITIONAL_WORK_BYTES", _lib.CONDITIONAL_WORK_BYTES), \
            chunked_calls.replaced(_lib, "blockwise_chunk", two_per_call), \
            chunked_calls.spied(lib, "sc_blockwise_granger_f64", 11, 12) as calls:
        chunked, _ = c.blockwise_spectral_granger_prediction(CHUNK_LABELS)
    return dict(chunked=squeeze(chunked), whole=squeeze(whole), status=c._last_wilson["status"], calls=np.array(calls))


def check_chunked(r, S, precision, host):
    """Four calls across the two batches into one output: against the reference and against the unchunked run of the same
    object, both within bounds(); statuses [6 pairs, 1 group]."""
    assert r["calls"].tolist() == [[2, 3], [1, 3], [2, 4], [1, 4]], r["calls"]
    assert r["status"].shape == (6, 1) and (r["status"] == 1).all()
    print(f"blockwise Granger, {host} host, {precision}: chunked == unchunked bit for bit:",
          np.array_equal(r["chunked"], r["whole"], equal_nan=True))
    ref, _ = bref.blockwise_granger(S, CHUNK_LABELS)
    assert_close(r["chunked"], ref, *bounds(precision), what="chunked vs reference")
    assert_close(r["chunked"], r["whole"], *bounds(precision), what="chunked vs unchunked")


def test_block_pairs_in_chunks(_engine_precision):
    """Seven signals in groups of 2, 2, 2, 1 whose block pairs go two per call: BLOCKWISE_KEEP_OUTPUT across calls and batches and
    the offsets of the member / split / cell lists and of n_iter / status, which the 4 GB default bound never exercises."""
    S = cref.var_spectrum(*random_var(7, 22), 32)
    check_chunked(chunked_and_whole(S), S, _engine_precision, "PyTorch")


def test_block_pairs_in_chunks_on_the_torch_free_host(_engine_precision):
    S = cref.var_spectrum(*random_var(7, 22), 32)
    r = chunked_calls.on_torch_free_host("test_gpu_blockwise_granger", "chunked_and_whole", _engine_precision, S=S)
    check_chunked(r, S, _engine_precision, "torch-free")
