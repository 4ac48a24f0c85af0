"""Connectivity.seed_jackknife on the device (sjk_kernel of sc_seed_jackknife.hip) against the NumPy float64 yardstick of
tests/seed_jackknife_ref.py -- jackknife_ref.jackknife and phase_lag_jackknife_ref.jackknife indexed at [..., seeds, targets] -- and
against the all-pairs Connectivity.jackknife and Connectivity.seed_connectivity of the same object.

Inputs are uploaded coefficients of phase_lag_jackknife_ref.lagged_noise and margin_phases; the reference gets the same coefficients
in float64.  PARITY_CASES are the smallest shapes at which each mechanism of the kernel can go wrong: two units, three signals, the
unit splits and their fold (50 and 1000 trials), a unit longer than a staging block (g = 35) and one that straddles blocks (g = 6),
both kinds of units, the largest seed list the interface takes (64 seeds: 16 chunks; against 258 targets of six observations it is
also the case with the most entries at the fewest observations, where the float32 engines' errors are widest), the edges of the
target tile -- 64 targets, and 128 for a request of two seeds (the plan's split of the four waves, sc_seed_jackknife.hip); 255 to
257 targets of one seed are there for the 256-target split the diagnostic switch selects and cost nothing as the fourth edge of
the 64-target tile --, the edges of the seed chunk (1, 4, 5 seeds), seeds that are the last signals
(seed index above target index), targets in descending and scattered order, a seed among the targets and targets=None.

Bounds.  Float64 engine: 1e-9 (1 + |ref|) on estimate and bias_corrected, 1e-9 relative on standard_error.  Float32 engines: F32_BOUNDS
below, see there.  NaN patterns must be equal; a standard error that is exactly 0 in the reference must be exactly 0 on the device.
On the float32 engines the PLI and the debiased PLI^2 are held to the yardstick on margin_phases only -- there they are sums of
integers and must agree to 1e-14 -- and not on lagged_noise, where a product whose Im s is of the order of its float32 rounding may
take either sign (tests/test_gpu_phase_lag_jackknife.py has the reason at length).  No other entry is left out of any comparison."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chunked_calls                                        # noqa: E402
import phase_lag_jackknife_ref as pref                      # noqa: E402
import seed_jackknife_ref as sjref                          # noqa: E402

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
# (the two-rank test starts its own processes, which run both engines themselves; the amplitude test drives the float32 engine)
SC_PRECISIONS_TESTS = ("test_parity", "test_margin_phases", "test_contract_with_the_all_pairs_jackknife",
                       "test_estimate_is_the_seed_measure", "test_mixed_requests_and_determinism",
                       "test_nothing_is_stored_outside_the_buffers", "test_the_abi_refuses_before_launching",
                       "test_torch_free_host_gives_the_same_values")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = sjref.OUTPUTS
SIX = sjref.MEASURES
COH, IMCOH, PLI, WPLI, DPLI2, DWPLI2 = SIX
INTEGER = (PLI, DPLI2)                      # sums of signs: exact on every engine while no sign can flip
NOT_INTEGER = (COH, IMCOH, WPLI, DWPLI2)

F64_BOUND = 1e-9
INTEGER_BOUND = 1e-14
# the bounds of the all-pairs jackknife tests (tests/test_gpu_jackknife.py, tests/test_gpu_phase_lag_jackknife.py), which these may
# never exceed
F32_CAPS = {"estimate": 2e-6, "bias_corrected": 8e-5, "standard_error": 1e-3}
F32_CAP_STANDARD_ERROR_MANY_UNITS = 5e-6
# 4 x the worst error of the float32 engines over PARITY_CASES on both makers against the float64 yardstick, measured on the MI355X
# (the FIGURE lines this file prints under `pytest -s`; profiles/seed_jackknife_accuracy.txt), one digit, and the cap where that is
# lower.  Measured (both float32 selections alike): estimate 5.6e-7 (4 x is 2.2e-6: the bound is the cap, 2e-6), bias_corrected
# 8.9e-7 (bound 4e-6), standard_error 8.6e-4 (the cap, 1e-3) -- all three for the debiased wPLI^2 at 64 seeds x 258 targets of three
# trials of two tapers, where a leave-one-out estimate has four observations (the all-pairs test has its worst at the same shape) --,
# standard_error with 50 and more delete units 2.9e-6 (4 x is 1.2e-5: the cap, 5e-6; debiased wPLI^2 at 1000 trials on margin_phases).
F32_BOUNDS = {"estimate": 2e-6, "bias_corrected": 4e-6, "standard_error": 1e-3}
F32_STANDARD_ERROR_MANY_UNITS = 5e-6          # 50 or more delete units
assert all(F32_BOUNDS[o] <= F32_CAPS[o] for o in OUTPUTS) and F32_STANDARD_ERROR_MANY_UNITS <= F32_CAP_STANDARD_ERROR_MANY_UNITS

WIDE = (1, 3, 2, 3, 258)                                          # 3 trials of 2 tapers, 258 signals
SCATTERED = (11, 3, 16, 0, 8, 5, 13, 1, 9)
# (W, R, K, F, C, expectation_type, over, seeds, targets)
PARITY_CASES = [
    (2, 2, 3, 5, 2, "trials_tapers", "trials", (1,), None),                                   # two units; seed above, seed as target
    (1, 3, 4, 5, 3, "trials_tapers", "trials", (2, 0), None),
    (2, 50, 3, 5, 16, "trials_tapers", "trials", (15, 14), None),                             # three unit splits; the last signals
    (1, 1000, 7, 9, 16, "trials_tapers", "trials", (3, 12), None),                            # many splits and the fold
    (5, 3, 7, 3, 3, "time_trials_tapers", "trials", (1,), None),                              # g = 35 > 32
    (3, 50, 2, 5, 17, "time_trials_tapers", "trials", (16, 2), tuple(range(16, -1, -1))),     # g = 6 straddles stagings; descending
    (2, 1, 7, 5, 16, "tapers", "observations", (5, 9), None),
    (1, 50, 3, 5, 17, "trials_tapers", "observations", (0,), SCATTERED),
    (1, 50, 3, 5, 17, "trials_tapers", "observations", (4, 16, 0), SCATTERED),
] + [WIDE + ("trials_tapers", "trials", (257, 0, 100), tuple(range(n))) for n in (63, 64, 65, 129)         # tile of 64 targets
] + [WIDE + ("trials_tapers", "trials", (257, 0), tuple(range(n))) for n in (127, 128, 129)                # tile of 128 targets
] + [WIDE + ("trials_tapers", "trials", (257,), tuple(range(n))) for n in (255, 256, 257)                  # one seed: fourth edge of the 64-tile
] + [(1, 3, 2, 3, 9, "trials_tapers", "trials", seeds, None) for seeds in ((4,), (8, 7, 6, 5), (8, 7, 6, 5, 0))   # chunk edges
] + [WIDE + ("trials_tapers", "trials", tuple(range(257, 1, -4)), None)]      # sc_seed_connectivity_max_seeds() = 64 seeds: 16 chunks
# margin_phases keeps |sin| of every phase difference above sin(3 pi / (4 (C + 1))) (asserted there): 0.069 at 33 signals and still
# 0.0091 at 258, four orders above the rounding of a float32 product (a few 2^-24), so no sign can flip at the wide shape either.
# Its tile-edge cases are here so that the float32 sign counts of the second and later tiles are held to the yardstick too.
MARGIN_CASES = [c for c in PARITY_CASES if c[4] <= 33 or len(c[7]) <= 3]


def case_id(c):
    return "-".join(str(v) for v in c[:7]) + f"-{len(c[7])}x{'all' if c[8] is None else len(c[8])}"


def n_units_of(case):
    W, R, K, _, _, expectation_type, over = case[:7]
    return R if over == "trials" else int(np.prod([(W, R, K)[a] for a in sjref.jref.EXPECTATION_AXES[expectation_type]]))


def bound(precision, output, n_units=2):
    if precision == "dtype":
        return F64_BOUND
    if output == "standard_error" and n_units >= 50:
        return F32_STANDARD_ERROR_MANY_UNITS
    return F32_BOUNDS[output]


def error(got, ref, output):
    """Worst error of one output in the units of its bound; NaN patterns must be equal (tests/test_gpu_jackknife.py's)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"shape {got.shape} != {ref.shape}"
    assert got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN patterns differ"
    ok = ~np.isnan(ref)
    if output == "standard_error":
        # purely relative; a standard error that is exactly 0 in the reference must be exactly 0 on the device too
        zero = ok & (ref == 0)
        assert np.all(got[zero] == 0), "a standard error that is exactly 0 in the reference is not 0 on the device"
        ok &= ~zero
        scale = np.abs(ref[ok])
    else:
        scale = 1 + np.abs(ref[ok])
    return float((np.abs(got[ok] - ref[ok]) / scale).max()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def coefficients_and_full_reference(shape, expectation_type, over, maker):
    """(coefficients, all-pairs reference of the six measures) of a shape, computed once for every engine and every seed list."""
    W, R, K, F, C = shape
    coef = getattr(pref, maker)(W, R, K, F, C, seed=C + R)
    coef.setflags(write=False)
    full = {}
    full.update(sjref.jref.jackknife(coef, expectation_type, sjref.FIRST, over))
    full.update(pref.jackknife(coef, expectation_type, pref.MEASURES, over))
    return coef, full


@functools.lru_cache(maxsize=None)
def inputs_and_reference(case, maker):
    coef, full = coefficients_and_full_reference(case[:5], case[5], case[6], maker)
    targets = np.arange(case[4]) if case[8] is None else np.asarray(case[8])
    ref = {m: {o: sjref.from_full(full[m][o], case[7], targets) for o in OUTPUTS} for m in SIX}
    for m in SIX:
        for o in OUTPUTS:
            ref[m][o].setflags(write=False)
    return coef, ref


def device(coef, case, measures=SIX):
    import spectral_connectivity_amd as sc
    c = sc.Connectivity(coef, expectation_type=case[5])
    return c, c.seed_jackknife(list(case[7]), None if case[8] is None else list(case[8]), measures, over=case[6])


def results_are_well_formed(res, case, measures=SIX):
    targets = np.arange(case[4]) if case[8] is None else np.asarray(case[8])
    assert np.array_equal(res.seeds, case[7]) and np.array_equal(res.targets, targets)
    assert res.seeds.dtype == res.targets.dtype == np.int32
    assert list(res.results) == [m for m in SIX if m in measures]
    own = np.asarray(case[7])[:, None] == targets[None, :]
    for m, r in res.results.items():
        assert (r.n_units, r.over, r.transform) == (n_units_of(case), case[6], "fisher_z" if m == COH else "identity")
        for o in OUTPUTS:
            assert getattr(r, o).shape[-3:] == (case[3], len(case[7]), len(targets))
            assert np.isnan(getattr(r, o)[..., own]).all(), f"{m} {o}: a seed that is its own target is NaN"


def check(got, ref, measures, precision, what, n_units, bounds=None):
    errors = {(m, o): error(getattr(got[m], o), ref[m][o] if isinstance(ref[m], dict) else getattr(ref[m], o), o)
              for m in measures for o in OUTPUTS}
    for (m, o), e in sorted(errors.items()):
        print(f"FIGURE {precision} | {what} | n_units {n_units} | {m} | {o} | {e:.3e}")
    for (m, o), e in errors.items():
        b = bounds(m, o) if bounds else bound(precision, o, n_units)
        assert e <= b, f"{what}: {m} {o} error {e:.3e} > {b:.1e}"


@pytest.mark.parametrize("case", PARITY_CASES, ids=case_id)
def test_parity(case, _engine_precision, request):
    precision = request.node.callspec.params["_engine_precision"]
    coef, ref = inputs_and_reference(case, "lagged_noise")
    _, res = device(coef, case)
    results_are_well_formed(res, case)
    check(res.results, ref, SIX if precision == "dtype" else NOT_INTEGER, precision, f"lagged_noise {case_id(case)}", n_units_of(case))


@pytest.mark.parametrize("case", MARGIN_CASES, ids=case_id)
def test_margin_phases(case, _engine_precision, request):
    precision = request.node.callspec.params["_engine_precision"]
    coef, ref = inputs_and_reference(case, "margin_phases")
    _, res = device(coef, case)
    results_are_well_formed(res, case)
    n = n_units_of(case)
    check(res.results, ref, SIX, precision, f"margin_phases {case_id(case)}", n,
          bounds=lambda m, o: INTEGER_BOUND if m in INTEGER else bound(precision, o, n))


def test_contract_with_the_all_pairs_jackknife(_engine_precision, request):
    """On one object: seed_jackknife(...) is jackknife(...) indexed at the seeds and targets -- the sign of x_seed conj(x_target),
    NaN where a seed is its own target -- within the bounds of the parity tests."""
    import spectral_connectivity_amd as sc
    precision = request.node.callspec.params["_engine_precision"]
    C = 33
    seeds, targets = [32, 5, 17], [0, 32, 31, 4, 5, 6, 20, 17, 16]
    for maker, expectation_type, over, R in (("lagged_noise", "trials_tapers", "trials", 7), ("margin_phases", "trials_tapers", "observations", 4)):
        coef = getattr(pref, maker)(2, R, 3, 5, C, seed=31)
        c = sc.Connectivity(coef, expectation_type=expectation_type)
        full = c.jackknife(SIX, over=over)
        res = c.seed_jackknife(seeds, targets, SIX, over=over)
        ref = {m: {o: sjref.from_full(getattr(full[m], o), seeds, targets) for o in OUTPUTS} for m in SIX}
        n = full[COH].n_units
        assert res.results[COH].n_units == n
        check(res.results, ref, SIX, precision, f"all-pairs jackknife {maker} over {over}", n)
        for m in sjref.ANTISYMMETRIC:                         # seed 32 against target 0 is minus the all-pairs entry (0, 32)
            assert np.array_equal(np.sign(res.results[m].estimate[..., 0, 0]), -np.sign(full[m].estimate[..., 0, 32])), m
        for m in SIX:
            for o in OUTPUTS:
                assert np.isnan(getattr(res.results[m], o)[..., [0, 1, 2], [1, 4, 7]]).all(), (m, o)


def lagged_series(T=512, R=12, C=6, seed=4):
    """Channel j is channel j - 1 delayed by 3 samples plus noise."""
    rng = np.random.default_rng(seed)
    x = np.empty((T + 3 * C, R, C))
    x[:, :, 0] = rng.standard_normal((T + 3 * C, R))
    for j in range(1, C):
        x[:, :, j] = np.roll(x[:, :, j - 1], 3, axis=0) + 0.7 * rng.standard_normal((T + 3 * C, R))
    return x[3 * C:]


def on_the_statistics_scale(name, value):
    value = np.asarray(value, dtype=np.float64)
    return np.arctanh(np.sqrt(value)) if name == COH else value


@pytest.mark.parametrize("expectation_type", ["trials_tapers", "time_trials_tapers"])
def test_estimate_is_the_seed_measure(expectation_type, _engine_precision, request):
    """``estimate`` is seed_connectivity's value of the same name on the statistic's scale, off the NaN entries (the imaginary
    coherence of the methods is an absolute value: the estimate's is compared)."""
    import spectral_connectivity_amd as sc
    precision = request.node.callspec.params["_engine_precision"]
    C = 6
    m = sc.Multitaper(lagged_series(C=C), sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=128)
    c = sc.Connectivity.from_multitaper(m, expectation_type=expectation_type)
    seeds, targets = [5, 1], [0, 1, 2, 3, 4]
    res = c.seed_jackknife(seeds, targets, SIX)
    values = c.seed_connectivity(seeds, targets, SIX).values
    own = np.asarray(seeds)[:, None] == np.asarray(targets)[None, :]
    b = bound(precision, "estimate")
    for name in SIX:
        want = on_the_statistics_scale(name, values[name]).copy()
        want[..., own] = np.nan
        got = res.results[name].estimate
        if name == DWPLI2:                                   # a real series: NaN at the zero and Nyquist bins, in both
            assert np.isnan(got[..., [0, -1], :, :]).all()
        e = error(np.abs(got) if name == IMCOH else got, want, "estimate")
        print(f"FIGURE {precision} | estimate against seed_connectivity | {expectation_type} | {name} | {e:.3e}")
        assert e <= b, name
    assert np.abs(res.results[WPLI].estimate[..., 1:-1, :, :][..., ~own]).max() > 0.5        # (the lag shows)


def same_bits(a, b, what):
    for o in OUTPUTS:
        assert np.array_equal(getattr(a, o), getattr(b, o), equal_nan=True), f"{what} {o}"
    assert (a.transform, a.n_units, a.over) == (b.transform, b.n_units, b.over), what


def test_mixed_requests_and_determinism(_engine_precision):
    """One call with six names is six calls with one, bit for bit; two runs are bit-identical; a second request on the same object
    reads the cached totals again -- no second totals pass -- and gives the same bits."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import _lib
    lib = _lib.load()
    coef = pref.lagged_noise(2, 40, 2, 5, 19, seed=17)            # 40 trials: two unit splits
    seeds, targets = [18, 3], [0, 18, 7, 2]
    suffix = "_f64" if _engine_precision == "dtype" else "_f32"
    for over in ("trials", "observations"):
        c = sc.Connectivity(coef, expectation_type="trials_tapers")
        with chunked_calls.spied(lib, "sc_seed_jackknife_totals" + suffix, 6) as totals:
            six = c.seed_jackknife(seeds, targets, SIX[::-1], over=over).results
            assert list(six) == list(SIX) and totals == [0x2F]
            again = c.seed_jackknife(seeds, targets, SIX, over=over).results
            for m in SIX:
                same_bits(six[m], again[m], f"{over} {m}: second request on the cached totals")
                same_bits(six[m], c.seed_jackknife(seeds, targets, (m,), over=over).results[m], f"{over} {m} alone, cached totals")
            assert totals == [0x2F], "a request the cached totals cover ran the totals pass again"
            c.seed_jackknife(seeds, None, (WPLI,), over=over)
            assert totals == [0x2F, 0x3], "other targets need totals of their own"
        fresh = sc.Connectivity(coef, expectation_type="trials_tapers")
        for m in SIX:                                          # (totals with the planes of this measure alone)
            same_bits(six[m], fresh.seed_jackknife(seeds, targets, (m,), over=over).results[m], f"{over} {m} alone")
        rerun = sc.Connectivity(coef, expectation_type="trials_tapers").seed_jackknife(seeds, targets, SIX, over=over).results
        for m in SIX:
            same_bits(six[m], rerun[m], f"{over} {m}: two runs")


def abi_inputs(coef, expectation_type, n_freq):
    import spectral_connectivity_amd as sc
    c = sc.Connectivity(coef, expectation_type=expectation_type)
    sp = c._device()
    return c, sp, sp.desc(expectation_type, n_freq)


def test_nothing_is_stored_outside_the_buffers(_engine_precision):
    """The two drivers on guarded memory (tests/guarded_buffers.py): the workspaces of split calls, the totals record and the output
    lie between bands of a pattern, which survive.  70 targets and 5 seeds: a ragged last tile and a short last chunk.  Then an index
    outside [0, C) handed to the ABI directly: it counts as a signal of zeros -- no load, no fault."""
    import torch
    from guarded_buffers import guarded_memory
    from spectral_connectivity_amd import _lib, _stage_d, engine
    lib = _lib.load()
    C, F = 72, 5
    coef = pref.lagged_noise(1, 40, 2, F, C, seed=29)
    c, sp, d = abi_inputs(coef, "trials_tapers", F)
    seeds, targets = np.array([71, 3, 9, 0, 40], dtype=np.int32), np.arange(70, dtype=np.int32)[::-1].copy()
    planes, mask = 0x2F, 0x3F

    def run(mem, seeds=seeds, targets=targets):
        total = _stage_d.seed_jackknife_totals(mem, sp, "trials_tapers", seeds, targets, planes, 0, n_freq=F)
        out, n_bins = _stage_d.seed_jackknife(mem, sp, "trials_tapers", seeds, targets, total, planes, mask, 0, 40, n_freq=F)
        return total, out

    want = run(engine.TorchMemory(torch.device("cuda:0")))
    mem = guarded_memory()
    got = run(mem)
    torch.cuda.synchronize()
    ws_t = int(lib.sc_seed_jackknife_totals_workspace_bytes(ctypes.byref(d), 5, 70, planes, 0, 0, 40))
    ws_j = int(lib.sc_seed_jackknife_workspace_bytes(ctypes.byref(d), 5, 70, mask, 0, 0, 40))
    assert ws_t > 0 and ws_j > 0 and ws_t in mem.sizes() and ws_j in mem.sizes()
    assert F * _lib.seed_record_doubles(5, 70, planes) * 8 in mem.sizes() and 6 * 3 * F * 5 * 70 * 8 in mem.sizes()
    assert mem.intact(), "stored outside a workspace, the record or the output"
    for g, w in zip(got, want):
        assert torch.equal(g.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), "differs from the ordinary host path"
    # indices outside [0, C): seed 1 and targets 2 and 4 of the lists; the in-range entries are those of the clean lists
    bad_seeds, bad_targets = np.array([71, C, 9], dtype=np.int32), np.array([69, 5, -1, 0, C + 1000000, 71], dtype=np.int32)
    mem = guarded_memory()
    total, out = run(mem, bad_seeds, bad_targets)
    torch.cuda.synchronize()
    assert mem.intact()
    _, clean = run(engine.TorchMemory(torch.device("cuda:0")), bad_seeds[[0, 2]], bad_targets[[0, 1, 3, 5]])
    out = out.cpu().numpy().reshape(6, 3, F, 3, 6)[:, :, :, [0, 2]][..., [0, 1, 3, 5]]
    assert np.array_equal(out, clean.cpu().numpy().reshape(6, 3, F, 2, 4), equal_nan=True)
    rec = total.cpu().numpy()
    assert np.isfinite(rec).all()
    cells = rec[:, :5 * 18].reshape(F, 5, 3, 6)
    assert np.all(cells[:, :, 1] == 0) and np.all(cells[:, :, :, [2, 4]] == 0), "a signal of zeros sums to 0"
    assert np.all(rec[:, 5 * 18 + 1] == 0) and np.all(rec[:, 5 * 18 + 3 + 2] == 0) and np.all(rec[:, 5 * 18 + 3 + 4] == 0)


def test_the_abi_refuses_before_launching(_engine_precision):
    """A totals record without a plane a requested measure reads, a workspace one byte short and a unit range outside the spectra
    are SC_EINVAL with real device pointers too, and the output is untouched."""
    import torch
    from guarded_buffers import guarded_memory
    from spectral_connectivity_amd import _lib, _stage_d
    lib = _lib.load()
    F, R = 5, 40
    coef = pref.lagged_noise(1, R, 2, F, 6, seed=3)
    c, sp, d = abi_inputs(coef, "trials_tapers", F)
    mem = guarded_memory()
    seeds = np.array([5, 2], dtype=np.int32)
    d_seeds = mem.upload(seeds)
    planes = _lib.PLANE_CSM | _lib.SEED_PLANE_POWER
    total = _stage_d.seed_jackknife_totals(mem, sp, "trials_tapers", seeds, None, planes, 0, n_freq=F)
    ws_bytes = int(lib.sc_seed_jackknife_workspace_bytes(ctypes.byref(d), 2, 6, 0x9, 0, 0, R))
    assert ws_bytes > 0
    ws, out = mem.empty((ws_bytes,), np.uint8), mem.empty((2 * 3 * F * 2 * 6,), np.float64)
    fn = lib.sc_seed_jackknife_f64 if sp.f64 else lib.sc_seed_jackknife_f32

    def call(planes=planes, mask=0x3, lo=0, hi=R, ws_bytes=ws_bytes):
        return fn(mem.ptr(sp.X), ctypes.byref(d), mem.ptr(d_seeds), 2, None, 6, mem.ptr(total), planes, mask, 0, lo, hi, R, mem.ptr(out),
                  mem.ptr(ws), ws_bytes, mem.stream())

    assert call(mask=0x9) == -1 and b"lacks a plane" in lib.sc_last_error()            # wPLI: no |Im s| plane in the record
    assert call(mask=0x4) == -1 and b"lacks a plane" in lib.sc_last_error()            # PLI: no sign plane
    assert call(ws_bytes=int(lib.sc_seed_jackknife_workspace_bytes(ctypes.byref(d), 2, 6, 0x3, 0, 0, R)) - 1) == -1
    assert b"workspace too small" in lib.sc_last_error()
    assert call(hi=R + 1) == -1 and b"unit range" in lib.sc_last_error()
    assert call(lo=3, hi=3) == -1 and b"unit range" in lib.sc_last_error()
    tot = lib.sc_seed_jackknife_totals_f64 if sp.f64 else lib.sc_seed_jackknife_totals_f32
    rec = mem.empty(tuple(total.shape), np.float64)
    assert tot(mem.ptr(sp.X), ctypes.byref(d), mem.ptr(d_seeds), 2, None, 6, planes, 0, 0, R + 1, mem.ptr(rec), mem.ptr(ws), ws_bytes,
               mem.stream()) == -1 and b"unit range" in lib.sc_last_error()
    assert tot(mem.ptr(sp.X), ctypes.byref(d), mem.ptr(d_seeds), 2, None, 6, planes, 0, 0, R, mem.ptr(rec), mem.ptr(ws),
               int(lib.sc_seed_jackknife_totals_workspace_bytes(ctypes.byref(d), 2, 6, planes, 0, 0, R)) - 1, mem.stream()) == -1
    assert b"workspace too small" in lib.sc_last_error()
    torch.cuda.synchronize()
    assert mem.intact()
    untouched = [bool((buf[4096:4096 + n] == 0x5A).all()) for buf, n in mem.buffers]
    assert untouched[-3:] == [True, True, True], "a refused call wrote to its workspace, its output or its record"
    assert call() == 0                                                                    # (the same arguments, nothing wrong: runs)
    torch.cuda.synchronize()
    assert mem.intact() and np.isfinite(out.cpu().numpy().reshape(2, 3, F, 2, 6)[..., 0, :5]).all()


def seed_jackknife_scenario(coef, seeds, targets):
    """(runs in the child process of test_torch_free_host_gives_the_same_values, and in the test itself on the PyTorch host)"""
    import spectral_connectivity_amd as sc
    out = {}
    for over in ("trials", "observations"):
        res = sc.Connectivity(coef).seed_jackknife([int(s) for s in seeds], [int(t) for t in targets], SIX, over=over)
        out.update({f"{over}.{m}.{o}": getattr(r, o) for m, r in res.results.items() for o in OUTPUTS})
    try:
        sc.Connectivity(np.ones((1, 2, 1, 8, 257), dtype=complex)).seed_jackknife([0])
        out["refused"] = np.array("")
    except ValueError as exc:
        out["refused"] = np.array(str(exc))
    return out


def test_torch_free_host_gives_the_same_values(_engine_precision):
    """The same drivers on the torch-free host, in a process that never imports torch: the bits of the PyTorch host, and that
    host's limit of 256 signals."""
    coef = pref.lagged_noise(2, 9, 3, 5, 9, seed=23)
    seeds, targets = [7, 2, 4], [8, 2, 0, 7, 5]
    there = chunked_calls.on_torch_free_host("test_gpu_seed_jackknife", "seed_jackknife_scenario", _engine_precision, coef=coef,
                                             seeds=np.array(seeds), targets=np.array(targets))
    here = seed_jackknife_scenario(coef, seeds, targets)
    assert str(there["refused"]).startswith("seed_jackknife of more than 256 signals") and str(here["refused"]) == ""
    assert set(there) == set(here) and len(here) == 2 * 6 * 3 + 1
    for key in here:
        if key != "refused":
            assert np.array_equal(there[key], here[key], equal_nan=True), key


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU), 7 trials as 4 + 3: the totals records add over the ranks, every
    rank walks its own units against the sum, one all-reduce adds the stacked sums; the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29613",
                          os.path.join(ROOT, "tools", "check_sharded_seed_jackknife.py")],
                         env=env, capture_output=True, text=True, timeout=300)
    print("\n".join(line for line in out.stdout.splitlines() if line.startswith("FIGURE")))
    assert out.returncode == 0 and "sharded seed jackknife OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_amplitude_guard():
    """A series in tesla (x 1e-13) on the float32 engine: (Im s)^2 leaves the float32 range, the request is walked on the complex128
    copy (_guard_spectra) and the debiased wPLI^2 jackknife is that of the same series scaled to order 1, within the float32 bounds."""
    import spectral_connectivity_amd as sc
    from spectral_connectivity_amd import _lib
    lib = _lib.load()
    x = lagged_series(T=384, R=6, C=6, seed=9)
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=128)
    seeds, targets = [5, 0], [1, 2, 3, 4, 5]
    res = {}
    for scale in (1.0, 1e-13):
        c = sc.Connectivity.from_multitaper(sc.Multitaper(x * scale, **kw), dtype=np.complex64)
        with chunked_calls.spied(lib, "sc_seed_jackknife_f64", 3) as wide, chunked_calls.spied(lib, "sc_seed_jackknife_f32", 3) as narrow:
            res[scale] = c.seed_jackknife(seeds, targets, (DWPLI2,)).results[DWPLI2]
        assert (wide, narrow) == (([2], []) if scale < 1 else ([], [2])), "the out-of-range request did not go through the complex128 copy"
    assert np.isfinite(res[1.0].estimate[..., 1:-1, :, :][..., [0, 0, 0, 0, 1, 1, 1, 1], [0, 1, 2, 3, 0, 1, 2, 3]]).all()
    for o in OUTPUTS:
        e = error(getattr(res[1e-13], o), getattr(res[1.0], o), o)
        print(f"FIGURE float32 | debiased wPLI^2 at 1e-13 against order 1 | {o} | {e:.3e}")
        assert e <= F32_BOUNDS[o], o
