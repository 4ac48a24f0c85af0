"""Connectivity.seed_connectivity (csrc/sc_seed.hip) on the device, against the oracle's ten all-pairs functions indexed
[..., seeds, :][..., targets] and against the all-pairs method of the same object.

Bounds, in the form of close32 of tests/test_gpu_parity.py (|a - b| <= tol |b| + tol max |b|): float32 engine 1e-5, 3e-5 for PLV /
PPC, 1e-4 for the two debiased measures; float64 engine 1e-9; equal NaN pattern, equal infinities.  The coherence phase is held to
the all-pairs method without exception; against the oracle the entries on the oracle's branch cut (branch_cut) are taken modulo
2 pi.  The shapes are the smallest at
which each mechanism of the kernel can go wrong: the edges of the 64-target tile (1, 63, 64, 65, 257 targets of 258 signals), of the
4-seed chunk (1, 2, 3, 4, 5 and sc_seed_connectivity_max_seeds() seeds), of the 32-row block (1, 2, 31, 32, 33, 65 observations),
and the observation split (5 bins, 600 observations).  One observation leaves the pairwise phase consistency out: (|u|^2 - 1) / 0
of a unit phasor u is +-inf or NaN by the rounding of |u|^2, in the reference too."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chunked_calls                                        # noqa: E402
import seed_connectivity_ref as sref                        # noqa: E402
from guarded_buffers import guarded_memory                  # noqa: E402
from oracle import spectral_oracle as so                    # noqa: E402

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
# (the two-rank test starts its own processes, which run both engines themselves; the amplitude test drives the float32 engine)
SC_PRECISIONS_TESTS = ("test_target_tile_edges", "test_seed_chunk_edges", "test_row_block_edges", "test_observation_split",
                       "test_every_expectation_type", "test_channel_without_power_and_zero_coefficient", "test_targets_permuted_and_subset_seeds_unsorted", "test_one_pass",
                       "test_from_multitaper", "test_nothing_is_stored_outside_the_buffers", "test_torch_free_host")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURES = sref.MEASURES
F32_BOUNDS = dict({m: 1e-5 for m in MEASURES}, phase_locking_value=3e-5, pairwise_phase_consistency=3e-5,
                  debiased_squared_phase_lag_index=1e-4, debiased_squared_weighted_phase_lag_index=1e-4)
NO_PPC = tuple(m for m in MEASURES if m != "pairwise_phase_consistency")


def bound(precision, name):
    return 1e-9 if precision == "dtype" else F32_BOUNDS[name]


def close(a, b, tol, what, cut=None):
    """``cut``: entries of a phase that lie on the branch cut of the ORACLE (branch_cut): compared modulo 2 pi."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs ({np.isnan(a).sum()} vs {np.isnan(b).sum()})"
    inf = np.isinf(b)
    assert np.array_equal(a[inf], b[inf]), f"{what}: infinities differ"
    ok = np.isfinite(b)
    if not ok.any():
        return 0.0
    scale = np.abs(b[ok]).max()
    err = np.abs(a[ok] - b[ok])
    if cut is not None:
        err = np.where(cut[ok], np.abs((a[ok] - b[ok] + np.pi) % (2 * np.pi) - np.pi), err)
    worst = (err / np.maximum(tol * np.abs(b[ok]) + tol * scale, 1e-300)).max()
    print(f"FIGURE {what}: max err {err.max():.3e} (scale {scale:.3e}), worst err / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: max err {err.max():.3e} (scale {scale:.3e}), worst err/bound {worst:.2f}"
    return worst


def branch_cut(name, coherency):
    """Where the oracle's cross-spectrum is real and negative -- every observation real, as at the zero and Nyquist bins of a real
    series -- its phase is +pi or -pi by the sign of a zero: NumPy's depends on the signs of the factors, the device's on the side
    of the diagonal (above: +0, below: the negated entry above).  These entries of the ORACLE comparison, and no others, are taken
    modulo 2 pi; the comparison with the all-pairs method of the same object is exact everywhere."""
    if name != "coherence_phase":
        return None
    return (np.asarray(coherency).imag == 0) & (np.asarray(coherency).real < 0)


@functools.lru_cache(maxsize=None)
def coefficients(W, R, K, N, C, seed):
    rng = np.random.default_rng(seed)
    coef = rng.standard_normal((W, R, K, N, C)) + 1j * rng.standard_normal((W, R, K, N, C))
    coef.setflags(write=False)
    return coef


@functools.lru_cache(maxsize=None)
def oracle(shape_seed, expectation_type, name):
    with np.errstate(invalid="ignore", divide="ignore"):
        out = getattr(so, name)(coefficients(*shape_seed), expectation_type)
    out.setflags(write=False)
    return out


def check(precision, shape_seed, seeds, targets, expectation_type="trials_tapers", measures=MEASURES, full=True):
    """One call for all of ``measures``; every value against the oracle and (``full``) against the method of the same object."""
    import spectral_connectivity_amd as sc
    coef = coefficients(*shape_seed)
    c = sc.Connectivity(coef, expectation_type=expectation_type)
    res = c.seed_connectivity(seeds, targets, measures)
    t = np.arange(coef.shape[-1]) if targets is None else np.asarray(targets)
    assert list(res.values) == list(measures)
    assert np.array_equal(res.seeds, seeds) and np.array_equal(res.targets, t)
    for name in measures:
        tag = f"{name} {shape_seed} {len(seeds)} seeds {len(t)} targets {expectation_type}"
        close(res.values[name], sref.from_full(oracle(shape_seed, expectation_type, name), seeds, t), bound(precision, name),
              tag + " | oracle", branch_cut(name, sref.from_full(oracle(shape_seed, expectation_type, "coherency"), seeds, t)))
        if full:
            mine = getattr(c, name)()
            assert res.values[name].dtype == mine.dtype, (name, res.values[name].dtype, mine.dtype)
            close(res.values[name], sref.from_full(mine, seeds, t), bound(precision, name), tag + " | all-pairs method")
    return c, res


BIG = (1, 3, 2, 8, 258, 11)          # 6 observations of 258 signals, 5 bins


@pytest.mark.parametrize("n_targets", [1, 63, 64, 65, 257])
def test_target_tile_edges(_engine_precision, n_targets):
    # seed 0 is among the targets, seed 257 is not; the all-pairs methods of 258 signals are compared once, at 257 targets
    check(_engine_precision, BIG, [257, 0], list(range(n_targets)), full=n_targets == 257)


@pytest.mark.parametrize("n_seeds", [1, 2, 3, 4, 5, 64])
def test_seed_chunk_edges(_engine_precision, n_seeds):
    from spectral_connectivity_amd import _lib
    assert _lib.load().sc_seed_connectivity_max_seeds() == 64
    shape = (1, 3, 2, 8, 70, 12)
    seeds = [int(s) for s in np.random.default_rng(n_seeds).permutation(70)[:n_seeds]]          # not in ascending order
    check(_engine_precision, shape, seeds, None, full=n_seeds in (5, 64))                       # targets=None: every seed is a target


@pytest.mark.parametrize("n_obs", [1, 2, 31, 32, 33, 65])
def test_row_block_edges(_engine_precision, n_obs):
    check(_engine_precision, (1, n_obs, 1, 8, 6, 13), [4, 1], None, measures=NO_PPC if n_obs == 1 else MEASURES)


def test_channel_without_power_and_zero_coefficient(_engine_precision):
    """Channel 2 is zero everywhere (the eps floors, weights below eps, 0 / 0 unit phasors, sign 0, the debiased wPLI NaN), and one
    coefficient of channel 4 is zero (its unit phasor is 0 * inf = NaN in that observation: PLV and PPC of that bin and channel NaN):
    as seeds and as targets, against the oracle and the methods."""
    import spectral_connectivity_amd as sc
    coef = np.array(coefficients(1, 6, 2, 8, 6, 18))
    coef[..., 2] = 0.0
    coef[0, 3, 1, 2, 4] = 0.0
    c = sc.Connectivity(coef)
    for seeds, targets in (([2, 0], None), ([4, 1], [0, 4, 2, 3])):
        res = c.seed_connectivity(seeds, targets, MEASURES)
        t = np.arange(6) if targets is None else np.asarray(targets)
        for name in MEASURES:
            with np.errstate(invalid="ignore", divide="ignore"):
                ref = sref.from_full(getattr(so, name)(coef), seeds, t)
            tol = bound(_engine_precision, name)
            close(res.values[name], ref, tol, f"{name} degenerate {seeds} | oracle")
            close(res.values[name], sref.from_full(getattr(c, name)(), seeds, t), tol, f"{name} degenerate {seeds} | all-pairs method")
        assert np.isnan(res.values["phase_locking_value"]).any() and not np.isnan(res.values["phase_locking_value"]).all()


def test_observation_split(_engine_precision):
    """One kept group of 5 bins and 600 observations: bins x tiles cannot fill the device, the observations are split over
    workgroups whose partial records are added in split order -- the same bits on every run."""
    from spectral_connectivity_amd import _lib
    shape = (1, 600, 1, 8, 5, 14)
    c, first = check(_engine_precision, shape, [3, 0], None, "time_trials_tapers")
    d = c._device().desc("time_trials_tapers", 5)
    assert _lib.load().sc_seed_accumulate_workspace_bytes(ctypes.byref(d), 2, 5, 0x3F) > 0
    again = c.seed_connectivity([3, 0], None, MEASURES)
    for name in MEASURES:
        assert np.array_equal(first.values[name], again.values[name], equal_nan=True), name


@pytest.mark.parametrize("expectation_type", list(sref.EXPECTATION_AXES))
def test_every_expectation_type(_engine_precision, expectation_type):
    """Three windows, four trials, three tapers: every expectation type averages at least three observations.  With two, the
    debiased wPLI is 2 i1 i2 / (2 |i1| |i2|) = +-1 through two complete cancellations, and the comparison with the all-pairs method
    would test the float32 engine's all-pairs RECORDS, whose float32 sums lose i_max / i_min x 6e-8 of it (measured with two tapers,
    840 entries: the seed values within 9.5e-13 of the oracle, the all-pairs method 3.6e-4 away from both); two observations
    against the oracle and the method are in test_row_block_edges."""
    _, res = check(_engine_precision, (3, 4, 3, 8, 7, 15), [5, 0], None, expectation_type)
    kept = tuple(n for i, n in enumerate((3, 4, 3)) if i not in sref.EXPECTATION_AXES[expectation_type])
    assert res.values["coherency"].shape == kept + (5, 2, 7)


def test_targets_permuted_and_subset_seeds_unsorted(_engine_precision):
    shape = (2, 5, 3, 16, 9, 16)
    check(_engine_precision, shape, [7, 2, 4], [8, 2, 0, 7, 5])
    check(_engine_precision, shape, [3], [3])
    _, a = check(_engine_precision, shape, [0], [1], measures=("weighted_phase_lag_index", "phase_lag_index", "coherence_phase"))
    _, b = check(_engine_precision, shape, [1], [0], measures=("weighted_phase_lag_index", "phase_lag_index", "coherence_phase"))
    for name in a.values:                       # the sign is that of x_seed conj(x_target)
        close(a.values[name], -b.values[name], bound(_engine_precision, name), name + " antisymmetry")
        assert np.abs(a.values[name]).max() > 0.01


def test_one_pass(_engine_precision):
    """All ten measures, three accumulator families and the powers: ONE call of the accumulate entry point, one of the epilogue,
    and no all-pairs accumulator."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import _lib
    lib = _lib.load()
    c = sc.Connectivity(coefficients(1, 3, 2, 8, 70, 12))
    name = "sc_seed_accumulate_f64" if _engine_precision == "dtype" else "sc_seed_accumulate_f32"
    other = "sc_seed_accumulate_f32" if _engine_precision == "dtype" else "sc_seed_accumulate_f64"
    with chunked_calls.spied(lib, name, 3, 5, 6) as calls, chunked_calls.spied(lib, other, 3) as others, \
            chunked_calls.spied(lib, "sc_seed_measure_f64", 8) as epilogues:
        c.seed_connectivity(list(range(64)), None, MEASURES)
    assert calls == [(64, 70, 0x3F)] and others == [] and epilogues == [10]
    assert not c._accum_cache, "an all-pairs accumulator was created"


FS, NW, L, STEP, T = 200.0, 3, 64, 32, 192


@functools.lru_cache(maxsize=None)
def series():
    rng = np.random.default_rng(17)
    x = rng.standard_normal((T + 40, 6, 20))
    for j in range(1, 20):                                   # channel j is channel j - 1 delayed by 2 samples plus noise
        x[:, :, j] = np.roll(x[:, :, j - 1], 2, axis=0) + 0.8 * rng.standard_normal((T + 40, 6))
    x = x[40:]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def series_oracle(name, scale=1.0):
    coef, _ = so.multitaper_fft(series() * scale, fs=FS, NW=NW, n_time_samples_per_window=L, n_time_samples_per_step=STEP)
    with np.errstate(invalid="ignore", divide="ignore"):
        return getattr(so, name)(coef)


def test_from_multitaper(_engine_precision):
    """A real series of 20 channels: zero and Nyquist bins (Im s = 0 in every observation: sign 0, the debiased wPLI NaN where the
    method is NaN).  The all-pairs methods run first, so that under the planes format the seed call reads decoded spectra."""
    import spectral_connectivity_amd as sc
    m = sc.Multitaper(series(), sampling_frequency=FS, time_halfbandwidth_product=NW, n_time_samples_per_window=L,
                      n_time_samples_per_step=STEP)
    c = sc.Connectivity.from_multitaper(m)
    seeds, targets = [19, 3], list(range(20))
    full = {name: getattr(c, name)() for name in MEASURES}
    res = c.seed_connectivity(seeds, None, MEASURES)
    assert np.isnan(res.values["debiased_squared_weighted_phase_lag_index"][:, 0]).all()
    assert np.isnan(res.values["debiased_squared_weighted_phase_lag_index"][:, -1]).all()
    assert (res.values["phase_lag_index"][:, 0] == 0).all()
    for name in MEASURES:
        tol = bound(_engine_precision, name)
        assert res.values[name].dtype == full[name].dtype, name
        ref = sref.from_full(series_oracle(name), seeds, targets)
        cut = branch_cut(name, sref.from_full(series_oracle("coherency"), seeds, targets))
        close(res.values[name], ref, tol, name + " from_multitaper | oracle", cut)
        if cut is not None:              # (real negative cross-spectra exist in this series: the method's sign of pi is tested)
            assert cut.any()
        close(res.values[name], sref.from_full(full[name], seeds, targets), tol, name + " from_multitaper | all-pairs method")


def test_amplitude_guard():
    """The same series in tesla (x 1e-13) on the float32 engine: (Im s)^2 leaves the float32 range, the request is accumulated from
    the complex128 copy (_guard_spectra) and the debiased wPLI and PLV stay within their bounds."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import _lib
    m = sc.Multitaper(series() * 1e-13, sampling_frequency=FS, time_halfbandwidth_product=NW, n_time_samples_per_window=L,
                      n_time_samples_per_step=STEP)
    c = sc.Connectivity.from_multitaper(m, dtype=np.complex64)
    names = ("debiased_squared_weighted_phase_lag_index", "phase_locking_value")
    lib = _lib.load()
    with chunked_calls.spied(lib, "sc_seed_accumulate_f64", 3) as wide, chunked_calls.spied(lib, "sc_seed_accumulate_f32", 3) as narrow:
        res = c.seed_connectivity([19, 3], None, names)
    assert wide == [2] and narrow == [], "the out-of-range request did not go through the complex128 copy"
    for name in names:
        assert res.values[name].dtype == np.float32
        close(res.values[name], sref.from_full(series_oracle(name, 1e-13), [19, 3], list(range(20))), F32_BOUNDS[name],
              name + " at 1e-13")


def test_nothing_is_stored_outside_the_buffers(_engine_precision):
    """The driver on guarded memory (tests/guarded_buffers.py): the workspace of a split call, the record and the ten outputs lie
    between bands of a pattern, which survive; the outputs are the bits of the ordinary path."""
    import torch
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import _lib, _stage_d, engine
    c = sc.Connectivity(coefficients(1, 600, 1, 8, 5, 14), expectation_type="time_trials_tapers")
    sp = c._device()
    codes = [_lib.SEED_MEASURES[m][0] for m in MEASURES]
    wide = [c._wide_output(code) for code in codes]
    seeds, targets = np.array([3, 0], dtype=np.int32), np.array([4, 0, 2], dtype=np.int32)

    def run(mem):
        return _stage_d.seed_connectivity(mem, sp, "time_trials_tapers", seeds, targets, 0x3F, codes, wide, n_freq=5)

    want = run(engine.TorchMemory(torch.device("cuda:0")))
    mem = guarded_memory()
    got = run(mem)
    torch.cuda.synchronize()
    ws = int(_lib.load().sc_seed_accumulate_workspace_bytes(ctypes.byref(sp.desc("time_trials_tapers", 5)), 2, 3, 0x3F))
    assert ws > 0 and ws in mem.sizes() and 5 * _lib.seed_record_doubles(2, 3, 0x3F) * 8 in mem.sizes()
    assert mem.intact(), "stored outside the workspace, the record or an output"
    for name, g, w in zip(MEASURES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), f"{name} differs from the ordinary host path"


def seed_scenario(coef, seeds, targets):
    """(runs in the child process of test_torch_free_host, and in the test itself on the PyTorch host)"""
    import spectral_connectivity_amd as sc
    res = sc.Connectivity(coef).seed_connectivity([int(s) for s in seeds], [int(t) for t in targets], MEASURES)
    out = dict(res.values)
    try:
        sc.Connectivity(np.ones((1, 2, 1, 8, 257), dtype=complex)).seed_connectivity([0])
        out["refused"] = np.array("")
    except ValueError as exc:
        out["refused"] = np.array(str(exc))
    return out


def test_torch_free_host(_engine_precision):
    """The same driver on the torch-free host, in a process that never imports torch: the values of the PyTorch host, and the
    jackknife's limit of 256 signals there."""
    shape = (2, 5, 3, 16, 9, 16)
    seeds, targets = [7, 2, 4], [8, 2, 0, 7, 5]
    there = chunked_calls.on_torch_free_host("test_gpu_seed_connectivity", "seed_scenario", _engine_precision, coef=coefficients(*shape),
                                             seeds=np.array(seeds), targets=np.array(targets))
    here = seed_scenario(coefficients(*shape), seeds, targets)
    assert "more than 256 signals" in str(there["refused"]) and str(here["refused"]) == ""
    for name in MEASURES:
        assert there[name].dtype == here[name].dtype, name
        close(there[name], here[name], bound(_engine_precision, name), name + " torch-free host | PyTorch host")
        close(there[name], sref.from_full(oracle(shape, "trials_tapers", name), seeds, targets), bound(_engine_precision, name),
              name + " torch-free host | oracle",
              branch_cut(name, sref.from_full(oracle(shape, "trials_tapers", "coherency"), seeds, targets)))


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU), 5 trials as 3 + 2: the seed records add over the ranks, every rank
    runs the epilogue; the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29597",
                          os.path.join(ROOT, "tools", "check_sharded_seed_connectivity.py")],
                         env=env, capture_output=True, text=True, timeout=300)
    print("\n".join(line for line in out.stdout.splitlines() if line.startswith("FIGURE")))
    assert out.returncode == 0 and "sharded seed connectivity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
