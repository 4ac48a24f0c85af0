"""Connectivity.jackknife on the device (sc_jackknife.hip) against the NumPy float64 reference of tests/jackknife_ref.py.

Inputs are seeded mixed complex Gaussian noise (jackknife_ref.mixed_noise) as uploaded coefficients, and Multitaper objects of
mixed white noise; the reference gets the same coefficients in float64.

Bounds.  Float64 engine: 1e-9 * (1 + |ref|) on estimate, bias_corrected and standard_error.  Float32 engines: 4 x the worst
error measured on the MI355X over PARITY_CASES on both float32 selections (the FIGURE lines this file prints under `pytest -s`;
DESIGN.md section 4.11, profiles/jackknife_accuracy.txt), rounded
up to one digit -- estimate and bias_corrected relative to 1 + |ref|, the standard error purely relative and never above 1e-3.
Measured: estimate 4.4e-7 (bound 2e-6), bias_corrected 2.0e-5 (bound 8e-5; worst under "trials" with 3 trials, where a
leave-one-out coherence of two observations lies close to 1), standard_error 3.7e-4 (4 x would be 1.5e-3: the bound is the cap,
1e-3; worst with two trials, where the standard error is |d_1 - d_2| / 2, a difference of two deviations that share most of
their value -- with 50 and more units the worst is 1.0e-6).
Cases with 50 or more delete units have a standard-error bound of their own, 5e-6 (measured worst 1.0e-6 x 4, rounded up).
Two device results that should agree (permuted trials, a rescaled channel, trial shards, the measure's own method) are held to
the same bound, once.

Under "trials" with two trials a leave-one-out estimate is ONE observation, whose coherence is identically 1 (arctanh = inf, or
whatever the rounding of |s| / sqrt(p p) makes of it): the statistic does not exist there and the reference itself returns
rounding noise, so the parity cases run "trials" with 3 and 50 trials and their two-trial cases use expectations with several
tapers; test_two_trials_one_observation_each checks power and the imaginary coherence, which do exist there, and the warning."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jackknife_ref as jref

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
# (the two-rank test starts its own processes, which run both engines themselves)
SC_PRECISIONS_TESTS = ("test_parity", "test_from_multitaper", "test_estimate_is_the_transformed_measure", "test_invariances",
                       "test_306_channels", "test_one_call_equals_three", "test_zero_power_channel",
                       "test_two_trials_one_observation_each", "test_duplicated_channel",
                       "test_torch_free_host_gives_the_same_values", "test_torch_free_host_from_multitaper")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("estimate", "bias_corrected", "standard_error")
THREE = ("power", "coherence_magnitude", "imaginary_coherence")

F64_BOUND = 1e-9
# 4 x the measured worst of the float32 engines: estimate / bias_corrected relative to 1 + |ref|, standard
# error relative
F32_BOUNDS = {"estimate": 2e-6, "bias_corrected": 8e-5, "standard_error": 1e-3}
F32_STANDARD_ERROR_MANY_UNITS = 5e-6          # 50 or more delete units (measured worst 1.0e-6)

# (W, R, K, F, C, expectation_type, over)
PARITY_CASES = [
    (2, 2, 3, 5, 2, "trials_tapers", "trials"),
    (1, 3, 4, 5, 3, "trials_tapers", "trials"),
    (2, 50, 3, 5, 16, "trials_tapers", "trials"),
    (1, 1000, 7, 9, 16, "trials_tapers", "trials"),
    (1, 50, 2, 3, 17, "trials_tapers", "trials"),
    (1, 3, 5, 3, 33, "trials_tapers", "trials"),
    (1, 50, 3, 3, 64, "trials_tapers", "trials"),
    (1, 3, 2, 3, 129, "trials_tapers", "trials"),
    (3, 50, 2, 5, 17, "time_trials_tapers", "trials"),
    (2, 2, 3, 5, 16, "time_trials_tapers", "trials"),
    (3, 50, 1, 3, 33, "time_trials", "trials"),
    (2, 50, 2, 5, 3, "trials", "trials"),
    (2, 3, 2, 5, 3, "trials", "trials"),
    (2, 1, 7, 5, 16, "tapers", "observations"),
    (1, 50, 3, 5, 17, "trials_tapers", "observations"),
    (1, 1000, 1, 5, 2, "trials", "observations"),
]


def bound(precision, output, n_units=2):
    if precision == "dtype":
        return F64_BOUND
    if output == "standard_error" and n_units >= 50:
        return F32_STANDARD_ERROR_MANY_UNITS
    return F32_BOUNDS[output]


def error(got, ref, output):
    """Worst error of one output in the units of its bound; NaN patterns must be equal."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"shape {got.shape} != {ref.shape}"
    assert got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN patterns differ"
    ok = ~np.isnan(ref)
    if output == "standard_error":
        # purely relative; a standard error that is exactly 0 (the imaginary coherence of a real series at the zero and Nyquist
        # bins: every unit's cross-spectrum is real there) must be exactly 0 on the device too
        zero = ok & (ref == 0)
        assert np.all(got[zero] == 0), "a standard error that is exactly 0 in the reference is not 0 on the device"
        ok &= ~zero
        scale = np.abs(ref[ok])
    else:
        scale = 1 + np.abs(ref[ok])
    return float((np.abs(got[ok] - ref[ok]) / scale).max())


def device(coef, expectation_type, measures=THREE, over="trials"):
    import spectral_connectivity_amd as sc
    return sc.Connectivity(coef, expectation_type=expectation_type).jackknife(measures, over=over)


def case_errors(case):
    """{(measure, output): error} of one parity case on the engine in force."""
    W, R, K, F, C, expectation_type, over = case
    coef = jref.mixed_noise(W, R, K, F, C, seed=C + R)
    got = device(coef, expectation_type, over=over)
    ref = jref.jackknife(coef, expectation_type, THREE, over)
    n = R if over == "trials" else int(np.prod([(W, R, K)[a] for a in jref.EXPECTATION_AXES[expectation_type]]))
    out = {}
    for m in THREE:
        assert got[m].n_units == n and got[m].over == over
        assert got[m].transform == {"power": "log", "coherence_magnitude": "fisher_z", "imaginary_coherence": "identity"}[m]
        for o in OUTPUTS:
            out[(m, o)] = error(getattr(got[m], o), ref[m][o], o)
    C_ = np.arange(C)
    assert np.isnan(got["coherence_magnitude"].estimate[..., C_, C_]).all()
    return out, n


def check(errors, precision, what, n_units=2):
    for (m, o), e in sorted(errors.items()):
        print(f"FIGURE {precision} | {what} | n_units {n_units} | {m} | {o} | {e:.3e}")
    for (m, o), e in errors.items():
        b = bound(precision, o, n_units)
        assert e <= b, f"{what}: {m} {o} error {e:.3e} > {b:.1e}"


@pytest.mark.parametrize("case", PARITY_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_parity(case, _engine_precision, request):
    errors, n = case_errors(case)
    check(errors, request.node.callspec.params["_engine_precision"], str(case), n)


def series(T, R, C, seed):
    rng = np.random.default_rng(seed)
    M = np.eye(C) + 0.4 * rng.standard_normal((C, C))
    return rng.standard_normal((T, R, C)) @ M.T


def multitaper(x, **kw):
    import spectral_connectivity_amd as sc
    kw = dict(dict(sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=64), **kw)
    return sc.Multitaper(x, **kw)


@pytest.mark.parametrize("coherence_first", [False, True])
@pytest.mark.parametrize("expectation_type", ["trials_tapers", "time_trials_tapers"])
def test_from_multitaper(expectation_type, coherence_first, _engine_precision, request):
    """Device-resident spectra; ``coherence_first``: the object has served coherence_magnitude() before, so a float32 transform
    has been asked for with a planes hint and (float32+planes) holds its spectra as f16 pieces."""
    import spectral_connectivity_amd as sc
    m = multitaper(series(256, 12, 6, 4))
    c = sc.Connectivity.from_multitaper(m, expectation_type=expectation_type)
    if coherence_first:
        c.coherence_magnitude()
    got = c.jackknife(THREE)
    ref = jref.jackknife(m.fft(), expectation_type, THREE)
    errors = {(k, o): error(getattr(got[k], o), ref[k][o], o) for k in THREE for o in OUTPUTS}
    check(errors, request.node.callspec.params["_engine_precision"], f"from_multitaper {expectation_type} first={coherence_first}")


def test_estimate_is_the_transformed_measure(_engine_precision):
    import spectral_connectivity_amd as sc
    coef = jref.mixed_noise(2, 20, 3, 9, 7, seed=11)
    c = sc.Connectivity(coef, expectation_type="trials_tapers")
    got = c.jackknife(THREE)
    b = bound(_engine_precision, "estimate")
    # (coherence_magnitude() is the SQUARED magnitude of the coherency, as in the reference; the Fisher-z statistic is arctanh of
    #  the magnitude itself)
    for name, want in (("power", np.log(c.power())), ("coherence_magnitude", np.arctanh(np.sqrt(c.coherence_magnitude()))),
                       ("imaginary_coherence", c.imaginary_coherence())):
        est = got[name].estimate
        if name == "imaginary_coherence":
            est = np.abs(est)
            want = want.copy()                         # (imaginary_coherence() has a 0 diagonal, the jackknife a NaN one)
            assert np.all(want[..., np.arange(7), np.arange(7)] == 0)
            want[..., np.arange(7), np.arange(7)] = np.nan
        e = error(est, want, "estimate")
        print(f"FIGURE {_engine_precision} | estimate against the measure | {name} | {e:.3e}")
        assert e <= b, name


def test_invariances(_engine_precision):
    coef = jref.mixed_noise(2, 30, 3, 5, 6, seed=13)
    a = device(coef, "trials_tapers")
    perm = np.random.default_rng(13).permutation(30)
    p = device(coef[:, perm], "trials_tapers")
    scaled = coef.copy()
    scaled[..., 2] *= 1000.0
    s = device(scaled, "trials_tapers")
    again = device(coef, "trials_tapers")
    shift = np.zeros(6)
    shift[2] = 2 * np.log(1000.0)
    for m in THREE:
        for o in OUTPUTS:
            assert np.array_equal(getattr(a[m], o), getattr(again[m], o), equal_nan=True), f"{m} {o}: two runs differ"
            b = bound(_engine_precision, o)
            e = error(getattr(p[m], o), getattr(a[m], o), o)
            print(f"FIGURE {_engine_precision} | permuted trials | {m} | {o} | {e:.3e}")
            assert e <= b, f"permuted trials: {m} {o} {e:.3e}"
            want = getattr(a[m], o) + (shift if m == "power" and o != "standard_error" else 0.0)
            e = error(getattr(s[m], o), want, o)
            print(f"FIGURE {_engine_precision} | channel scaled by 1000 | {m} | {o} | {e:.3e}")
            assert e <= b, f"channel scaled by 1000: {m} {o} {e:.3e}"


def test_306_channels(_engine_precision):
    """Beyond every per-launch channel limit of the stage-B kernels: the jackknife kernel tiles the channels itself."""
    W, R, K, F, C = 1, 8, 3, 9, 306
    coef = jref.mixed_noise(W, R, K, F, C, seed=306)
    got = device(coef, "trials_tapers")
    ref = jref.jackknife(coef, "trials_tapers", THREE)
    check({(m, o): error(getattr(got[m], o), ref[m][o], o) for m in THREE for o in OUTPUTS}, _engine_precision, "306 channels")


def test_two_trials_one_observation_each(caplog, _engine_precision):
    """"trials" with two trials: a leave-one-out estimate is one observation.  Power and the imaginary coherence exist there and
    are held to the reference; the coherence magnitude of one observation is identically 1, so asking for it warns once."""
    import logging
    import spectral_connectivity_amd as sc
    coef = jref.mixed_noise(2, 2, 3, 5, 6, seed=29)
    c = sc.Connectivity(coef, expectation_type="trials")
    with caplog.at_level(logging.WARNING):
        got = c.jackknife(("power", "imaginary_coherence"))
    assert not [r for r in caplog.records if "single observation" in r.getMessage()]
    ref = jref.jackknife(coef, "trials", ("power", "imaginary_coherence"))
    check({(m, o): error(getattr(got[m], o), ref[m][o], o) for m in ref for o in OUTPUTS}, _engine_precision, "two trials")
    with caplog.at_level(logging.WARNING):
        c.jackknife(("coherence_magnitude",))
    assert len([r for r in caplog.records if "single observation" in r.getMessage()]) == 1


def test_duplicated_channel(_engine_precision):
    """Two identical channels: their coherence magnitude is 1 up to the rounding of |S_ij| (1 / sqrt S_ii) (1 / sqrt S_jj), so the
    entries of THAT pair are arctanh of a number within a few ulp of 1 -- at least 17, inf or NaN -- in ``estimate`` and carry no
    promise in the other two outputs (the reference's own value there is rounding too); the pair's imaginary coherence is 0 up
    to the rounding of a fused x_i conj(x_i) (exactly 0 in the reference).  Every other entry is unaffected: held to the
    reference with the pair's two entries of the two C x C measures set aside."""
    coef = jref.mixed_noise(1, 12, 3, 5, 5, seed=31)
    coef[..., 3] = coef[..., 1]
    got = device(coef, "trials_tapers")
    ref = jref.jackknife(coef, "trials_tapers", THREE)
    est = got["coherence_magnitude"].estimate
    for i, j in ((1, 3), (3, 1)):
        pair = est[..., i, j]
        assert np.all(~np.isfinite(pair) | (pair >= 17.0)), pair
        assert np.all(np.abs(got["imaginary_coherence"].estimate[..., i, j]) <= bound(_engine_precision, "estimate"))
    errors = {}
    for m in THREE:
        for o in OUTPUTS:
            a, b = np.array(getattr(got[m], o)), np.array(ref[m][o])
            if m != "power":
                for x in (a, b):
                    x[..., 1, 3] = x[..., 3, 1] = np.nan
            errors[(m, o)] = error(a, b, o)
    check(errors, _engine_precision, "duplicated channel")


def test_one_call_equals_three(_engine_precision):
    import spectral_connectivity_amd as sc
    coef = jref.mixed_noise(2, 40, 2, 5, 19, seed=17)
    c = sc.Connectivity(coef, expectation_type="trials_tapers")
    for over in ("trials", "observations"):
        together = c.jackknife(THREE, over=over)
        for m in THREE:
            alone = c.jackknife((m,), over=over)[m]
            for o in OUTPUTS:
                assert np.array_equal(getattr(alone, o), getattr(together[m], o), equal_nan=True), f"{over} {m} {o}"


def test_zero_power_channel(caplog, _engine_precision):
    """A channel without power gives NaN in its entries and one counted warning."""
    import logging
    coef = jref.mixed_noise(1, 6, 2, 3, 4, seed=19)
    coef[..., 1] = 0.0
    with caplog.at_level(logging.WARNING):
        got = device(coef, "trials_tapers")
    ref = jref.jackknife(coef, "trials_tapers", THREE)
    for m in THREE:
        for o in OUTPUTS:
            error(getattr(got[m], o), ref[m][o], o)                  # (shapes and NaN patterns)
    assert np.isnan(got["power"].estimate[..., 1]).all() and np.isfinite(got["power"].estimate[..., 0]).all()
    msgs = [r.getMessage() for r in caplog.records if r.getMessage().startswith("jackknife:")]
    assert len(msgs) == 1 and msgs[0].startswith("jackknife: 3 entries of power are NaN")


def test_torch_free_host_gives_the_same_values(_engine_precision):
    coef = jref.mixed_noise(2, 9, 3, 5, 5, seed=23)
    here = device(coef, "trials_tapers")
    code = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import spectral_connectivity_amd as sc
from spectral_connectivity_amd import options
options.precision = sys.argv[2]
coef = np.load(sys.argv[3])
r = sc.Connectivity(coef, expectation_type="trials_tapers").jackknife(("power", "coherence_magnitude", "imaginary_coherence"))
np.savez(sys.argv[4], **{f"{m}.{o}": getattr(v, o) for m, v in r.items() for o in ("estimate", "bias_corrected", "standard_error")})
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cp, op = os.path.join(tmp, "coef.npy"), os.path.join(tmp, "out.npz")
        np.save(cp, coef)
        env = dict(os.environ, SC_HIP_HOST="numpy")
        out = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, cp, op], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "numpy host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        other = np.load(op)
        for m in THREE:
            for o in OUTPUTS:
                np.testing.assert_allclose(other[f"{m}.{o}"], getattr(here[m], o), rtol=1e-12, atol=1e-14, equal_nan=True)


def test_torch_free_host_from_multitaper(_engine_precision, request):
    """The torch-free host on device-resident spectra that have served coherence_magnitude() first (float32+planes: held as f16
    pieces and decoded once for the jackknife), against the reference run on that host's own m.fft()."""
    code = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import spectral_connectivity_amd as sc
from spectral_connectivity_amd import options
options.precision = sys.argv[2]
x = np.load(sys.argv[3])
m = sc.Multitaper(x, sampling_frequency=200.0, time_halfbandwidth_product=3, n_time_samples_per_window=64)
c = sc.Connectivity.from_multitaper(m)
c.coherence_magnitude()
r = c.jackknife(("power", "coherence_magnitude", "imaginary_coherence"))
out = {f"{k}.{o}": getattr(v, o) for k, v in r.items() for o in ("estimate", "bias_corrected", "standard_error")}
np.savez(sys.argv[4], fft=m.fft(), **out)
assert "torch" not in sys.modules
print("numpy host OK")
"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        xp, op = os.path.join(tmp, "x.npy"), os.path.join(tmp, "out.npz")
        np.save(xp, series(256, 12, 6, 4))
        env = dict(os.environ, SC_HIP_HOST="numpy")
        out = subprocess.run([sys.executable, "-c", code, ROOT, _engine_precision, xp, op], env=env, cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "numpy host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        other = np.load(op)
        ref = jref.jackknife(other["fft"], "trials_tapers", THREE)
        errors = {(m, o): error(other[f"{m}.{o}"], ref[m][o], o) for m in THREE for o in OUTPUTS}
    check(errors, request.node.callspec.params["_engine_precision"], "torch-free host from_multitaper")


def test_sharded_two_ranks_share_one_gpu():
    """parallel.ShardedConnectivity with 2 ranks (gloo, one GPU), 5 trials as 3 + 2: every rank walks its own units against the
    total record; the same values as one process."""
    env = dict(os.environ, SC_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29567",
                          os.path.join(ROOT, "tools", "check_sharded_jackknife.py")],
                         env=env, capture_output=True, text=True, timeout=600)
    print("\n".join(line for line in out.stdout.splitlines() if line.startswith("FIGURE")))
    assert out.returncode == 0 and "sharded jackknife OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
