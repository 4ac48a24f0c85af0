"""Connectivity.jackknife of the phase-lag family on the device (jk_phase_kernel of sc_jackknife.hip) against the NumPy float64
reference of tests/phase_lag_jackknife_ref.py.

Inputs are uploaded coefficients -- phase_lag_jackknife_ref.lagged_noise (complex mixing: a true wPLI that is not 0) and
margin_phases (every Im s keeps a relative margin of 0.069 from 0, so that no float32 rounding flips a sign) -- and Multitaper
objects of lagged series; the reference gets the same coefficients in float64.

Bounds.  Float64 engine: 1e-9 * (1 + |ref|) on estimate and bias_corrected, 1e-9 relative on standard_error.  Float32 engines:
4 x the worst error measured on the MI355X over PARITY_CASES and both input makers on both float32 selections (the FIGURE lines
this file prints under `pytest -s`; DESIGN.md section 4.11, profiles/phase_lag_jackknife_accuracy.txt), rounded up to one digit and
never above the bounds of the first jackknife family (tests/test_gpu_jackknife.py): F32_BOUNDS below.
Measured (wPLI and debiased wPLI^2, both makers): estimate 3.2e-7 (bound 2e-6), bias_corrected 1.4e-6 (bound 6e-6),
standard_error 4.8e-4 (4 x would be 1.9e-3: the bound is the cap, 1e-3; worst at 129 channels with three trials of two tapers,
where a leave-one-out estimate has four observations), and with 50 and more delete units 3.3e-6 (4 x would be 1.3e-5: the bound
is the cap, 5e-6; worst for the debiased wPLI^2 at 1000 trials on margin_phases, whose random phases make the true wPLI 0: a
pair there has |sum Im s| down to 2e-4 of sum |Im s|, and the rounding of the float32 products alone -- float64 sums, exact
totals -- gives 2.7e-6 in a NumPy model of the kernel, the rounding of the inputs to complex64 alone 1.6e-6).
On lagged_noise the float32 engines are held to the reference in the wPLI and the debiased wPLI^2 only: a product whose Im s is
of the order of its float32 rounding may take either sign, and with up to 63 000 products per entry too many entries would have
to be set aside; on margin_phases the PLI and the debiased PLI^2 are sums of integers that no engine can get wrong and are held
to 1e-9 on all of them.

A standard error that is exactly 0 in the reference must be exactly 0 on the device (the rule of tests/test_gpu_jackknife.py).
Three kinds of entries have one: the bins where Im s = 0 in every observation; a pair whose Im s has the same sign in every
observation (a handful of observations: wPLI = +-1 and debiased wPLI^2 = 1 in every delete-one set, because sum Im s =
+-sum |Im s| -- bit for bit on the device too, whose totals are the sums of its own unit sums); and a pair whose units all have
the same sign count, so that every unit has the same deviation (the kernel sums about the first unit's deviation)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import jackknife_ref as jref
import phase_lag_jackknife_ref as pref

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
# (the two-rank test starts its own processes, which run both engines themselves)
SC_PRECISIONS_TESTS = ("test_parity", "test_pli_is_exact_with_a_sign_margin", "test_estimate_is_the_measures_own_method",
                       "test_invariances", "test_constant_lag", "test_mixed_request", "test_torch_free_host_gives_the_same_values")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("estimate", "bias_corrected", "standard_error")
THREE = ("power", "coherence_magnitude", "imaginary_coherence")
FOUR = pref.MEASURES
PLI, WPLI, DPLI2, DWPLI2 = FOUR
INTEGER = (PLI, DPLI2)                      # sums of signs: exact on every engine while no sign can flip
WEIGHTED = (WPLI, DWPLI2)

F64_BOUND = 1e-9
# the bounds of the first family (tests/test_gpu_jackknife.py), which these may never exceed
F32_CAPS = {"estimate": 2e-6, "bias_corrected": 8e-5, "standard_error": 1e-3}
F32_CAP_STANDARD_ERROR_MANY_UNITS = 5e-6
# 4 x the measured worst of the float32 engines, one digit, capped (module docstring)
F32_BOUNDS = {"estimate": 2e-6, "bias_corrected": 6e-6, "standard_error": 1e-3}
F32_STANDARD_ERROR_MANY_UNITS = 5e-6          # 50 or more delete units
assert all(F32_BOUNDS[o] <= F32_CAPS[o] for o in OUTPUTS) and F32_STANDARD_ERROR_MANY_UNITS <= F32_CAP_STANDARD_ERROR_MANY_UNITS

# (W, R, K, F, C, expectation_type, over)
PARITY_CASES = [
    (2, 2, 3, 5, 2, "trials_tapers", "trials"),
    (1, 3, 4, 5, 3, "trials_tapers", "trials"),
    (2, 50, 3, 5, 16, "trials_tapers", "trials"),                # three unit splits
    (1, 1000, 7, 9, 16, "trials_tapers", "trials"),              # many splits and the fold
    (1, 50, 2, 3, 17, "trials_tapers", "trials"),
    (1, 3, 5, 3, 33, "trials_tapers", "trials"),
    (1, 50, 3, 3, 64, "trials_tapers", "trials"),
    (1, 3, 2, 3, 129, "trials_tapers", "trials"),
    (5, 3, 7, 3, 3, "time_trials_tapers", "trials"),             # g = 35 > 32
    (3, 50, 2, 5, 17, "time_trials_tapers", "trials"),           # g = 6 straddles stagings
    (2, 1, 7, 5, 16, "tapers", "observations"),
    (1, 50, 3, 5, 17, "trials_tapers", "observations"),
]
MARGIN_CASES = [c for c in PARITY_CASES if c[4] <= 33]


def case_id(c):
    return "-".join(str(v) for v in c)


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


def device(coef, expectation_type, measures=FOUR, over="trials"):
    import spectral_connectivity_amd as sc
    return sc.Connectivity(coef, expectation_type=expectation_type).jackknife(measures, over=over)


@functools.lru_cache(maxsize=None)
def inputs_and_reference(case, maker):
    """(coefficients, reference, n_units) of a case, computed once for the three engines."""
    W, R, K, F, C, expectation_type, over = case
    coef = getattr(pref, maker)(W, R, K, F, C, seed=C + R)
    ref = pref.jackknife(coef, expectation_type, FOUR, over)
    n = R if over == "trials" else int(np.prod([(W, R, K)[a] for a in jref.EXPECTATION_AXES[expectation_type]]))
    for m in FOUR:
        for o in OUTPUTS:
            ref[m][o].setflags(write=False)
    return coef, ref, n


def errors_against(got, ref, measures, precision):
    """{(measure, output): error} of device results against the reference."""
    return {(m, o): error(getattr(got[m], o), ref[m][o], o) for m in measures for o in OUTPUTS}


def check(errors, precision, what, n_units=2, bounds=None):
    for (m, o), e in sorted(errors.items()):
        print(f"FIGURE {precision} | {what} | n_units {n_units} | {m} | {o} | {e:.3e}")
    for (m, o), e in errors.items():
        b = bounds(m, o) if bounds else bound(precision, o, n_units)
        assert e <= b, f"{what}: {m} {o} error {e:.3e} > {b:.1e}"


def results_are_well_formed(got, n, over, C):
    idx = np.arange(C)
    for m in FOUR:
        assert got[m].n_units == n and got[m].over == over and got[m].transform == "identity"
        for o in OUTPUTS:
            assert np.isnan(getattr(got[m], o)[..., idx, idx]).all(), f"{m} {o}: the diagonal is NaN"
    assert list(got) == list(FOUR)


@pytest.mark.parametrize("case", PARITY_CASES, ids=case_id)
def test_parity(case, _engine_precision, request):
    precision = request.node.callspec.params["_engine_precision"]
    coef, ref, n = inputs_and_reference(case, "lagged_noise")
    got = device(coef, case[5], over=case[6])
    results_are_well_formed(got, n, case[6], case[4])
    measures = FOUR if precision == "dtype" else WEIGHTED
    check(errors_against(got, ref, measures, precision), precision, f"lagged_noise {case}", n)


@pytest.mark.parametrize("case", MARGIN_CASES, ids=case_id)
def test_pli_is_exact_with_a_sign_margin(case, _engine_precision, request):
    precision = request.node.callspec.params["_engine_precision"]
    coef, ref, n = inputs_and_reference(case, "margin_phases")
    got = device(coef, case[5], over=case[6])
    results_are_well_formed(got, n, case[6], case[4])
    check(errors_against(got, ref, FOUR, precision), precision, f"margin_phases {case}", n,
          bounds=lambda m, o: F64_BOUND if m in INTEGER else bound(precision, o, n))


def lagged_series(T=512, R=12, C=6, seed=4):
    """Channel j is channel j - 1 delayed by 3 samples plus noise."""
    rng = np.random.default_rng(seed)
    x = np.empty((T + 3 * C, R, C))
    x[:, :, 0] = rng.standard_normal((T + 3 * C, R))
    for j in range(1, C):
        x[:, :, j] = np.roll(x[:, :, j - 1], 3, axis=0) + 0.7 * rng.standard_normal((T + 3 * C, R))
    return x[3 * C:]


@pytest.mark.parametrize("expectation_type", ["trials_tapers", "time_trials_tapers"])
def test_estimate_is_the_measures_own_method(expectation_type, _engine_precision, request):
    import spectral_connectivity_amd as sc
    precision = request.node.callspec.params["_engine_precision"]
    C = 6
    m = sc.Multitaper(lagged_series(C=C), sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=128)
    c = sc.Connectivity.from_multitaper(m, expectation_type=expectation_type)
    before = {name: np.asarray(getattr(c, name)(), dtype=np.float64) for name in FOUR}
    got = c.jackknife(FOUR)
    after = {name: np.asarray(getattr(c, name)(), dtype=np.float64) for name in FOUR}
    idx, b = np.arange(C), bound(precision, "estimate")
    for name in FOUR:
        assert np.array_equal(before[name], after[name], equal_nan=True), f"{name}: the method's value changed with the jackknife"
        want = before[name].copy()
        want[..., idx, idx] = np.nan                       # (the methods have a 0 / finite diagonal, the jackknife a NaN one)
        e = error(got[name].estimate, want, "estimate")
        print(f"FIGURE {precision} | estimate against the measure | {expectation_type} | {name} | {e:.3e}")
        assert e <= b, name
    # a real series: Im s = 0 in every observation of the zero and the Nyquist bin
    off = ~np.eye(C, dtype=bool)
    for f in (0, -1):
        for name in (PLI, WPLI):
            for o in OUTPUTS:
                assert np.all(getattr(got[name], o)[..., f, :, :][..., off] == 0), f"{name} {o} bin {f}"
        for o in OUTPUTS:
            assert np.isnan(getattr(got[DWPLI2], o)[..., f, :, :]).all(), f"debiased wPLI^2 {o} bin {f}"
    assert np.isfinite(got[DWPLI2].estimate[..., 1:-1, :, :][..., off]).all()
    assert np.abs(got[WPLI].estimate[..., 1:-1, :, :][..., off]).max() > 0.5        # (the lag shows)


def test_invariances(_engine_precision, request):
    precision = request.node.callspec.params["_engine_precision"]
    C = 6
    coef = pref.margin_phases(2, 30, 3, 5, C, seed=13)
    a = device(coef, "trials_tapers")
    perm = np.random.default_rng(13).permutation(30)
    p = device(coef[:, perm], "trials_tapers")
    scaled = coef.copy()
    scaled[..., 2] *= 1000.0
    s = device(scaled, "trials_tapers")
    order = np.arange(C)
    order[[1, 4]] = order[[4, 1]]
    w = device(coef[..., order], "trials_tapers")
    for m in FOUR:
        for o in OUTPUTS:
            b = bound(precision, o)
            base = getattr(a[m], o)
            for what, other, want in (("permuted trials", p, base), ("channel scaled by 1000", s, base),
                                      ("channels 1 and 4 swapped", w, base[..., order, :][..., :, order])):
                e = error(getattr(other[m], o), want, o)
                print(f"FIGURE {precision} | {what} | {m} | {o} | {e:.3e}")
                assert e <= b, f"{what}: {m} {o} {e:.3e}"


def test_constant_lag(_engine_precision):
    """Every observation has the same sign of Im s for every pair: channel c leads channel c + 1 by 0.3 rad (+- 0.05)."""
    rng = np.random.default_rng(21)
    W, R, K, F, C = 2, 9, 3, 5, 4
    phase = rng.uniform(0, 2 * np.pi, (W, R, K, F, 1)) - 0.3 * np.arange(C) + rng.uniform(-0.05, 0.05, (W, R, K, F, C))
    coef = pref._two_sided(rng.uniform(0.5, 2.0, (W, R, K, F, C)) * np.exp(1j * phase))
    for over in ("trials", "observations"):
        got = device(coef, "trials_tapers", (PLI,), over=over)[PLI]
        i, j = np.triu_indices(C, 1)
        assert np.all(got.estimate[..., i, j] == 1.0) and np.all(got.estimate[..., j, i] == -1.0)
        off = ~np.eye(C, dtype=bool)
        assert np.all(got.standard_error[..., off] == 0)
        assert np.all((got.bias_corrected - got.estimate)[..., off] == 0)


def same_bits(a, b, what):
    for o in OUTPUTS:
        assert np.array_equal(getattr(a, o), getattr(b, o), equal_nan=True), f"{what} {o}"
    assert (a.transform, a.n_units, a.over) == (b.transform, b.n_units, b.over), what


def test_mixed_request(_engine_precision):
    import spectral_connectivity_amd as sc
    coef = pref.lagged_noise(2, 40, 2, 5, 19, seed=17)
    c = sc.Connectivity(coef, expectation_type="trials_tapers")
    for over in ("trials", "observations"):
        seven = c.jackknife(FOUR[::-1] + THREE[::-1], over=over)
        assert list(seven) == list(THREE) + list(FOUR)                  # (old names first, then new ones, each in table order)
        old, new = c.jackknife(THREE, over=over), c.jackknife(FOUR, over=over)
        again = c.jackknife(THREE + FOUR, over=over)
        for m in THREE:
            same_bits(seven[m], old[m], f"{over} {m}")
        for m in FOUR:
            same_bits(seven[m], new[m], f"{over} {m}")
            same_bits(seven[m], c.jackknife((m,), over=over)[m], f"{over} {m} alone")
        for m in THREE + FOUR:
            same_bits(seven[m], again[m], f"{over} {m}: two runs")


def test_torch_free_host_gives_the_same_values(_engine_precision):
    coef = pref.lagged_noise(2, 9, 3, 5, 5, seed=23)
    here = device(coef, "trials_tapers", THREE[2:] + FOUR)
    code = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import spectral_connectivity_amd as sc
from spectral_connectivity_amd import options
options.precision = sys.argv[2]
coef = np.load(sys.argv[3])
r = sc.Connectivity(coef, expectation_type="trials_tapers").jackknife(sys.argv[5].split(","))
np.savez(sys.argv[4], **{f"{m}.{o}": getattr(v, o) for m, v in r.items() for o in ("estimate", "bias_corrected", "standard_error")})
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cp, op = os.path.join(tmp, "coef.npy"), os.path.join(tmp, "out.npz")
        np.save(cp, coef)
        env = dict(os.environ, SC_HIP_HOST="numpy")
        out = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, cp, op, ",".join(THREE[2:] + FOUR)], env=env,
                             cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "numpy host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        other = np.load(op)
        for m in THREE[2:] + FOUR:
            for o in OUTPUTS:
                assert np.array_equal(other[f"{m}.{o}"], getattr(here[m], o), equal_nan=True), f"{m} {o}"


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU), 7 trials as 4 + 3: every rank walks its own units against the
    total record; the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29571",
                          os.path.join(ROOT, "tools", "check_sharded_phase_lag_jackknife.py")],
                         env=env, capture_output=True, text=True, timeout=300)
    print("\n".join(line for line in out.stdout.splitlines() if line.startswith("FIGURE")))
    assert out.returncode == 0 and "sharded phase-lag jackknife OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
