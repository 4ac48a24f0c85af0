"""CPU-only checks of the seed-jackknife boundary: the entry points of sc_seed_jackknife.hip are declared in include/sc_hip.h with
the argument types of _lib.py's ctypes prototypes and exported by libsc_hip.so, SC_ABI_VERSION is still 8, the layout and workspace
queries and the argument checks answer without a device, and Connectivity.seed_jackknife refuses a bad request before any device
work."""
import os
import re
from ctypes import POINTER, byref, c_double, c_int, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sc_seed_jackknife_layout": 9, "sc_seed_jackknife_workspace_bytes": 7, "sc_seed_jackknife_totals_workspace_bytes": 7,
         "sc_seed_jackknife_totals_f32": 14, "sc_seed_jackknife_totals_f64": 14, "sc_seed_jackknife_f32": 17,
         "sc_seed_jackknife_f64": 17}
SIX = tuple(_lib.SEED_JACKKNIFE_MEASURES)
ALL = 0x3F
CSM_POWER = _lib.PLANE_CSM | _lib.SEED_PLANE_POWER
ALL_PLANES = _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ | _lib.PLANE_SIGN_IM | _lib.SEED_PLANE_POWER


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_hip.h")).read(), flags=re.S)


def declaration(name):
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, f"{name} is not declared in sc_hip.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def ctype_of(arg):
    arg = re.sub(r"\bconst\b", "", arg).strip()
    if arg.startswith("sc_spectra_desc*"):
        return POINTER(_lib.SpectraDesc)
    if arg.startswith("int64_t*"):
        return POINTER(c_int64)
    if "*" in arg:
        return c_void_p
    return {"int64_t": c_int64, "uint32_t": c_uint32, "double": c_double, "int": c_int, "size_t": c_size_t}[arg.split()[0]]


@pytest.mark.parametrize("name", list(NAMES))
def test_header_matches_the_ctypes_prototype(name):
    ret, args = declaration(name)
    restype, argtypes = _lib.SYMBOLS[name]
    assert {"int": c_int, "int64_t": c_int64}[ret] is restype
    assert len(args) == len(argtypes) == NAMES[name]
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert ctype_of(arg) is want, f"{name} argument {i} ({arg}) is {want.__name__} in _lib.py"
    for stem in ("sc_seed_jackknife_totals", "sc_seed_jackknife"):
        assert declaration(stem + "_f32")[1][1:] == declaration(stem + "_f64")[1][1:]


def test_abi_version_and_constants():
    text = header()
    assert re.search(r"#define\s+SC_ABI_VERSION\s+8\b", text) and _lib.SC_ABI_VERSION == 8
    for name, (bit, transform, planes) in _lib.SEED_JACKKNIFE_MEASURES.items():
        short = {"phase_lag_index": "PLI", "weighted_phase_lag_index": "WPLI", "debiased_squared_phase_lag_index": "DEBIASED_PLI2",
                 "debiased_squared_weighted_phase_lag_index": "DEBIASED_WPLI2"}.get(name, name.upper())
        assert re.search(r"#define\s+SC_SEED_JACKKNIFE_" + short + r"\s+" + hex(bit) + r"u\b", text), name
        # the scale is that of the all-pairs jackknife, the planes those of the seed measure of the same name
        assert transform == (_lib.JACKKNIFE_MEASURES.get(name) or _lib.JACKKNIFE_PHASE_MEASURES[name])[1], name
        assert planes == _lib.SEED_MEASURES[name][1], name
    assert list(_lib.SEED_JACKKNIFE_MEASURES) == [k for k in _lib.JACKKNIFE_MEASURES if k != "power"] + list(_lib.JACKKNIFE_PHASE_MEASURES)
    assert "sc_seed_jackknife.hip" in _lib._build.SOURCES and os.path.exists(os.path.join(_lib._build.CSRC, "sc_seed_jackknife.hip"))
    for h in ("sc_jackknife_value.h", "sc_seed_layout.h"):
        assert h in _lib._build.HEADERS and os.path.exists(os.path.join(_lib._build.CSRC, h))


def desc(F=5, W=3, R=4, K=2, C=6, reduce=(0, 1, 1)):
    return _lib.SpectraDesc(n_freq=F, n_windows=W, n_trials=R, n_tapers=K, n_signals=C, stride_freq=W * R * K * C,
                            stride_window=R * K * C, stride_trial=K * C, stride_taper=C, reduce_window=reduce[0],
                            reduce_trial=reduce[1], reduce_taper=reduce[2], reserved=0)


def test_library_exports_and_layout_query():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    for name in NAMES:
        assert hasattr(lib, name)
    n_bins, n_units, unit_size, n_out = c_int64(), c_int64(), c_int64(), c_int64()
    d = desc()                                                      # 3 kept windows x 5 bins; 4 trials of 2 tapers
    for S, T in ((1, 1), (2, 6), (5, 65), (64, 257)):
        for mask in range(1, ALL + 1):
            assert lib.sc_seed_jackknife_layout(byref(d), S, T, mask, 0, byref(n_bins), byref(n_units), byref(unit_size), byref(n_out)) == 0
            assert (n_bins.value, n_units.value, unit_size.value) == (15, 4, 2)
            assert n_out.value == bin(mask).count("1") * 3 * 15 * S * T, (S, T, mask)
    assert lib.sc_seed_jackknife_layout(byref(d), 2, 6, ALL, 1, byref(n_bins), byref(n_units), byref(unit_size), byref(n_out)) == 0
    assert (n_units.value, unit_size.value) == (8, 1)
    assert lib.sc_seed_jackknife_layout(byref(d), 2, 6, ALL, 0, None, None, None, None) == 0
    kept_trials = desc(reduce=(1, 0, 1))
    for bad in ((byref(d), 0, 6, 1, 0), (byref(d), 65, 6, 1, 0), (byref(d), 2, 0, 1, 0), (byref(d), 2, 32769, 1, 0), (byref(d), 2, 6, 0, 0),
                (byref(d), 2, 6, 0x40, 0), (byref(d), 2, 6, 1, 2), (byref(kept_trials), 2, 6, 1, 0), (None, 2, 6, 1, 0)):
        assert lib.sc_seed_jackknife_layout(*bad, None, None, None, byref(n_out)) == -1, bad[1:]
    assert lib.sc_seed_jackknife_layout(byref(kept_trials), 2, 6, 1, 1, None, None, None, byref(n_out)) == 0       # (any expectation)


def test_workspace_queries_and_argument_checks_without_a_device():
    lib = _lib.load()
    per_bin, n_out = c_int64(), c_int64()
    full = desc(F=600, C=64)
    assert lib.sc_seed_jackknife_workspace_bytes(byref(full), 2, 64, ALL, 0, 0, 4) == 0          # bins fill the device: no split
    assert lib.sc_seed_jackknife_totals_workspace_bytes(byref(full), 2, 64, ALL_PLANES, 0, 0, 4) == 0
    # one kept group of 5 bins and 600 trials: the units are split, never fewer than 16 each, one partial output per split
    few = desc(F=5, W=1, R=600, K=1, C=20, reduce=(0, 1, 1))
    lib.sc_seed_jackknife_layout(byref(few), 2, 20, 0x9, 0, None, None, None, byref(n_out))
    ws = lib.sc_seed_jackknife_workspace_bytes(byref(few), 2, 20, 0x9, 0, 0, 600)
    n_splits, rem = divmod(ws, n_out.value * 8)
    assert rem == 0 and 2 <= n_splits <= 600 // 16, (ws, n_out.value)
    lib.sc_seed_record_layout(2, 20, ALL_PLANES, byref(per_bin))
    wt = lib.sc_seed_jackknife_totals_workspace_bytes(byref(few), 2, 20, ALL_PLANES, 0, 0, 600)
    assert wt == n_splits * 5 * per_bin.value * 8                    # the same splits: the query of either pass runs the one plan
    assert lib.sc_seed_jackknife_workspace_bytes(byref(few), 2, 20, 0x9, 0, 0, 31) == 0          # fewer than 32 units: one split
    for bad in ((0, 20, 0x9, 0, 0, 600), (2, 20, 0, 0, 0, 600), (2, 20, 0x9, 0, 0, 601), (2, 20, 0x9, 0, 5, 5), (2, 20, 0x9, 0, -1, 5)):
        assert lib.sc_seed_jackknife_workspace_bytes(byref(few), *bad) == 0, bad                 # (a failed plan has no workspace)
    assert lib.sc_seed_jackknife_totals_workspace_bytes(byref(few), 2, 20, _lib.PLANE_UNIT, 0, 0, 600) == 0

    fake = c_void_p(256)                 # never dereferenced: every check below returns before a launch
    d = desc()

    def refused(rc, *needles):
        assert rc == -1
        for needle in needles:
            assert needle in lib.sc_last_error(), lib.sc_last_error()

    for fn in (lib.sc_seed_jackknife_f32, lib.sc_seed_jackknife_f64):
        def call(X=fake, dsc=d, seeds=fake, S=2, T=6, total=fake, planes=ALL_PLANES, mask=ALL, over=0, lo=0, hi=4, n=4, out=fake,
                 ws=None, ws_bytes=0):
            return fn(X, byref(dsc) if dsc is not None else None, seeds, S, None, T, total, planes, mask, over, lo, hi, n, out, ws,
                      ws_bytes, None)
        refused(call(X=None), b"NULL")
        refused(call(dsc=None))
        refused(call(seeds=None), b"NULL")
        refused(call(total=None), b"NULL")
        refused(call(out=None), b"NULL")
        refused(call(S=0))
        refused(call(S=65))
        refused(call(T=0))
        refused(call(mask=0), b"measures")
        refused(call(mask=0x40), b"measures")
        refused(call(over=2), b"over")
        refused(call(dsc=desc(reduce=(1, 0, 1))), b"averages over trials")
        refused(call(lo=0, hi=5), b"unit range")                       # the spectra hold 4 trials
        refused(call(lo=2, hi=2), b"unit range")
        refused(call(lo=-1, hi=2), b"unit range")
        refused(call(hi=1, n=1), b"two units")
        refused(call(n=3), b"two units")                               # fewer units in the job than in this walk
        refused(call(planes=ALL_PLANES | _lib.PLANE_UNIT), b"planes")
        refused(call(planes=0x100), b"planes")
        # a total record that lacks a plane a requested measure reads
        refused(call(planes=_lib.PLANE_CSM, mask=0x1), b"lacks a plane")                       # coherence without the powers
        refused(call(planes=CSM_POWER, mask=0x4), b"lacks a plane")                            # PLI without the sign plane
        refused(call(planes=CSM_POWER | _lib.PLANE_SIGN_IM, mask=0x8), b"lacks a plane")       # wPLI without |Im s|
        refused(call(planes=CSM_POWER | _lib.PLANE_ABS_IM, mask=0x20), b"lacks a plane")       # debiased wPLI^2 without (Im s)^2
        # two units of one observation: a delete-one set holds one observation
        one = desc(F=5, W=1, R=2, K=1, C=6)
        refused(call(dsc=one, hi=2, n=2, mask=0x10), b"debiased")
        refused(call(dsc=one, hi=2, n=2, mask=0x20), b"debiased")
        # the workspace of a split call
        refused(call(dsc=few, T=20, mask=0x9, hi=600, n=600), b"workspace too small")
        refused(call(dsc=few, T=20, mask=0x9, hi=600, n=600, ws=fake, ws_bytes=ws - 1), b"workspace too small")
        refused(call(dsc=few, T=20, mask=0x9, hi=600, n=600, ws=c_void_p(264), ws_bytes=ws), b"16-byte aligned")
    for fn in (lib.sc_seed_jackknife_totals_f32, lib.sc_seed_jackknife_totals_f64):
        def call(X=fake, dsc=d, seeds=fake, S=2, T=6, planes=ALL_PLANES, over=0, lo=0, hi=4, rec=fake, ws=None, ws_bytes=0):
            return fn(X, byref(dsc) if dsc is not None else None, seeds, S, None, T, planes, over, lo, hi, rec, ws, ws_bytes, None)
        refused(call(X=None), b"NULL")
        refused(call(dsc=None))
        refused(call(seeds=None), b"NULL")
        refused(call(rec=None), b"NULL")
        refused(call(S=65))
        refused(call(T=32769))
        refused(call(planes=0), b"planes")
        refused(call(planes=_lib.SEED_PLANE_POWER), b"planes")
        refused(call(planes=_lib.PLANE_UNIT), b"planes")
        refused(call(over=3), b"over")
        refused(call(dsc=desc(reduce=(1, 0, 1))), b"averages over trials")
        refused(call(hi=5), b"unit range")
        refused(call(dsc=few, T=20, hi=600), b"workspace too small")
        refused(call(dsc=few, T=20, hi=600, ws=fake, ws_bytes=wt - 1), b"workspace too small")


def connectivity(shape=(1, 3, 2, 8, 70), expectation_type="trials_tapers"):
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(0)
    return sc.Connectivity(rng.standard_normal(shape) + 1j * rng.standard_normal(shape), expectation_type=expectation_type)


def test_bad_requests_raise_before_any_device_work():
    c = connectivity()
    for kwargs, match in ((dict(seeds=[0], measures=("coherence",)), "unknown measure"),
                          (dict(seeds=[0], measures=()), "measures is empty"),
                          (dict(seeds=[0], measures=("phase_lag_index", "phase_lag_index")), "twice"),
                          (dict(seeds=[0], measures=("coherence_magnitude", "imaginary_coherence", "coherence_magnitude")), "twice"),
                          (dict(seeds=[0], measures=("power",)), "'power' is not a measure of a"),
                          (dict(seeds=[0], measures=("coherence_magnitude", "power")), "'power' is not a measure of a"),
                          (dict(seeds=[0], measures=("phase_locking_value",)), "unknown measure"),
                          (dict(seeds=[0], over="windows"), "over must be"),
                          (dict(seeds=[]), "non-empty"),
                          (dict(seeds=[0], targets=[]), "non-empty"),
                          (dict(seeds=[70]), r"outside \[0, 70\)"),
                          (dict(seeds=[-1]), "outside"),
                          (dict(seeds=[0], targets=[3, 70]), "outside"),
                          (dict(seeds=[0.0]), "integers"),
                          (dict(seeds=[0], targets=[1.5]), "integers"),
                          (dict(seeds=[True]), "integers"),
                          (dict(seeds=[1, 2, 1]), "twice"),
                          (dict(seeds=[0], targets=[4, 5, 4]), "twice"),
                          (dict(seeds=list(range(65))), "at most 64 seeds")):
        with pytest.raises(ValueError, match=match):
            c.seed_jackknife(**kwargs)
    assert c._spectra is None and not c._accum_cache           # nothing was uploaded or accumulated
    kept = connectivity(expectation_type="tapers")
    with pytest.raises(ValueError, match="averages over trials"):
        kept.seed_jackknife([0], over="trials")
    one = connectivity((1, 1, 2, 8, 4))
    with pytest.raises(ValueError, match="n_trials >= 2"):
        one.seed_jackknife([0])
    with pytest.raises(ValueError, match="n_observations >= 2"):
        connectivity((1, 1, 1, 8, 4)).seed_jackknife([0], over="observations")
    two = connectivity((1, 2, 1, 8, 4))
    for name in ("debiased_squared_phase_lag_index", "debiased_squared_weighted_phase_lag_index"):
        for over in ("trials", "observations"):
            with pytest.raises(ValueError, match="at least two observations in a delete-one set"):
                two.seed_jackknife([0], measures=(name,), over=over)
    for obj in (kept, one, two):
        assert obj._spectra is None and not obj._accum_cache


def test_the_request_composes_the_three_existing_checks():
    seeds, targets, names, mask, planes, over_id, n_units = _lib.seed_jackknife_request(
        (3, 1), None, SIX[::-1], "trials", "trials_tapers", 5, 15, 8, 64)
    assert seeds.dtype == np.int32 and list(seeds) == [3, 1] and targets is None
    assert names == list(SIX) and mask == ALL and planes == ALL_PLANES and (over_id, n_units) == (0, 5)
    *_, names, mask, planes, over_id, n_units = _lib.seed_jackknife_request(
        [0], [2, 1], "weighted_phase_lag_index", "observations", "tapers", 5, 3, 8, 64)
    assert names == ["weighted_phase_lag_index"] and mask == 0x8 and planes == _lib.PLANE_CSM | _lib.PLANE_ABS_IM
    assert (over_id, n_units) == (1, 3)
    *_, names, mask, planes, _, _ = _lib.seed_jackknife_request([0], None, ("phase_lag_index", "imaginary_coherence"), "trials",
                                                                "trials", 4, 4, 8, 64)
    assert names == ["imaginary_coherence", "phase_lag_index"] and mask == 0x6 and planes == CSM_POWER | _lib.PLANE_SIGN_IM


def test_torch_free_host_refuses_more_than_256_signals():
    import subprocess
    import sys
    code = ("import sys\nimport numpy as np\nimport spectral_connectivity_amd as sc\n"
            "c = sc.Connectivity(np.ones((1, 2, 1, 8, 257), dtype=complex))\n"
            "try:\n    c.seed_jackknife([0])\nexcept ValueError as exc:\n    print('refused:', exc)\n"
            "assert 'torch' not in sys.modules\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, SC_HIP_HOST="numpy"))
    assert out.returncode == 0, out.stderr[-3000:]
    assert "refused: seed_jackknife of more than 256 signals" in out.stdout, out.stdout


def test_exports_and_wrapper():
    from spectral_connectivity_amd import connectivity, wrapper
    assert connectivity.SeedJackknife._fields == ("results", "seeds", "targets")
    assert "seed_jackknife" in wrapper._NOT_IN_DATASET
    with pytest.raises(ValueError, match="Connectivity class directly"):
        wrapper._check_method("seed_jackknife")
