"""CPU-only checks of the seed-connectivity boundary: the entry points of sc_seed.hip are declared in include/sc_hip.h with the
argument types of _lib.py's ctypes prototypes and exported by libsc_hip.so, SC_ABI_VERSION is still 8, the layout and workspace
queries and the argument checks answer without a device, and Connectivity.seed_connectivity refuses a bad request before any
device work."""
import os
import re
from ctypes import POINTER, byref, c_double, c_int, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"sc_seed_connectivity_max_seeds": 0, "sc_seed_record_layout": 4, "sc_seed_accumulate_workspace_bytes": 4,
         "sc_seed_accumulate_f32": 11, "sc_seed_accumulate_f64": 11, "sc_seed_measure_f64": 13}
ALL_PLANES = _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ | _lib.PLANE_SIGN_IM | _lib.PLANE_UNIT | _lib.SEED_PLANE_POWER


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_hip.h")).read(), flags=re.S)


def declaration(name):
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, f"{name} is not declared in sc_hip.h"
    args = [a.strip() for a in m.group(2).split(",")]
    return m.group(1), [] if args == ["void"] else args


def ctype_of(arg):
    arg = re.sub(r"\bconst\b", "", arg).strip()
    if arg.startswith("sc_spectra_desc*"):
        return (POINTER(_lib.SpectraDesc),)
    if arg.startswith("int64_t*"):
        return (POINTER(c_int64),)
    if arg.startswith("int*"):
        return (POINTER(c_int),)
    if arg.startswith("void* *") or arg.startswith("void**"):
        return (POINTER(c_void_p),)
    if "*" in arg:
        return (c_void_p,)
    base = arg.split()[0]
    return ({"int64_t": c_int64, "uint32_t": c_uint32, "double": c_double, "int": c_int, "size_t": c_size_t}[base],)


@pytest.mark.parametrize("name", list(NAMES))
def test_header_matches_the_ctypes_prototype(name):
    ret, args = declaration(name)
    restype, argtypes = _lib.SYMBOLS[name]
    assert {"int": c_int, "int64_t": c_int64}[ret] is restype
    assert len(args) == len(argtypes) == NAMES[name]
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{name} argument {i} ({arg}) is {want.__name__} in _lib.py"
    assert declaration("sc_seed_accumulate_f32")[1][1:] == declaration("sc_seed_accumulate_f64")[1][1:]


def test_abi_version_and_constants():
    text = header()
    assert re.search(r"#define\s+SC_ABI_VERSION\s+8\b", text) and _lib.SC_ABI_VERSION == 8
    assert re.search(r"#define\s+SC_SEED_PLANE_POWER\s+" + hex(_lib.SEED_PLANE_POWER) + "u", text)
    assert "sc_seed.hip" in _lib._build.SOURCES and os.path.exists(os.path.join(_lib._build.CSRC, "sc_seed.hip"))
    assert "sc_measure_value.h" in _lib._build.HEADERS
    # the planes of a measure are those of the method of the same name, plus the powers for the coherency family
    from spectral_connectivity_amd.connectivity import Connectivity
    for name, (code, planes) in _lib.SEED_MEASURES.items():
        assert planes & ~_lib.SEED_PLANE_POWER == Connectivity._METHOD_PLANES[name] == _lib.MEASURE_PLANES[code], name
        assert bool(planes & _lib.SEED_PLANE_POWER) == (name in ("coherency", "coherence_magnitude", "coherence_phase", "imaginary_coherence"))


def desc(F=5, W=3, R=4, K=2, C=6, reduce=(0, 1, 1)):
    return _lib.SpectraDesc(n_freq=F, n_windows=W, n_trials=R, n_tapers=K, n_signals=C, stride_freq=W * R * K * C,
                            stride_window=R * K * C, stride_trial=K * C, stride_taper=C, reduce_window=reduce[0],
                            reduce_trial=reduce[1], reduce_taper=reduce[2], reserved=0)


def test_library_exports_and_layout_query():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.sc_seed_connectivity_max_seeds() >= 64
    n = c_int64()
    for planes in range(1, ALL_PLANES + 1):
        for S, T in ((1, 1), (2, 308), (5, 65), (64, 257)):
            rc = lib.sc_seed_record_layout(S, T, planes, byref(n))
            if planes == _lib.SEED_PLANE_POWER:
                assert rc == -1                                       # the powers alone: no family to sum
                continue
            assert rc == 0 and n.value == _lib.seed_record_doubles(S, T, planes), (planes, S, T)
    assert _lib.seed_record_doubles(2, 308, _lib.PLANE_CSM | _lib.SEED_PLANE_POWER) == 2 * 2 * 308 + 2 + 308
    assert _lib.seed_record_doubles(3, 7, ALL_PLANES) == 7 * 21 + 10
    for bad in ((0, 4, 1), (65, 4, 1), (lib.sc_seed_connectivity_max_seeds() + 1, 4, 1), (2, 0, 1), (2, 32769, 1), (2, 4, 0), (2, 4, 0x40),
                (2, 4, 0x101)):
        assert lib.sc_seed_record_layout(*bad, byref(n)) == -1, bad
    assert lib.sc_seed_record_layout(2, 4, 1, None) == -1


def test_workspace_query_and_argument_checks_without_a_device():
    lib = _lib.load()
    planes = _lib.PLANE_CSM | _lib.SEED_PLANE_POWER
    n = c_int64()
    # bins x target tiles x seed chunks fill the device: no split, no workspace
    assert lib.sc_seed_accumulate_workspace_bytes(byref(desc(F=600, C=64)), 2, 64, planes) == 0
    # one kept group of 5 bins and 600 observations: the observations are split, one partial record per split
    few = desc(F=5, W=1, R=600, K=1, C=20, reduce=(0, 1, 1))
    lib.sc_seed_record_layout(2, 20, planes, byref(n))
    ws = lib.sc_seed_accumulate_workspace_bytes(byref(few), 2, 20, planes)
    n_splits, rem = divmod(ws, 5 * n.value * 8)
    assert rem == 0 and 2 <= n_splits <= 600 // 32, (ws, n.value)
    assert lib.sc_seed_accumulate_workspace_bytes(byref(few), 0, 20, planes) == 0          # (a failed plan has no workspace)
    fake = c_void_p(256)                 # never dereferenced: every check below returns before a launch
    d = desc()
    for fn in (lib.sc_seed_accumulate_f32, lib.sc_seed_accumulate_f64):
        assert fn(None, byref(d), fake, 2, None, 6, planes, fake, None, 0, None) == -1
        assert b"NULL" in lib.sc_last_error()
        assert fn(fake, None, fake, 2, None, 6, planes, fake, None, 0, None) == -1
        assert fn(fake, byref(d), None, 2, None, 6, planes, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, 2, None, 6, planes, None, None, 0, None) == -1
        assert fn(fake, byref(d), fake, 0, None, 6, planes, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, 65, None, 6, planes, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, 2, None, 0, planes, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, 2, None, 6, 0x40, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, 2, None, 6, _lib.SEED_PLANE_POWER, fake, None, 0, None) == -1
        assert fn(fake, byref(few), fake, 2, None, 20, planes, fake, None, 0, None) == -1
        assert b"workspace too small" in lib.sc_last_error()
        assert fn(fake, byref(few), fake, 2, None, 20, planes, fake, fake, ws - 1, None) == -1
        assert b"workspace too small" in lib.sc_last_error()
    one = (c_int * 1)(_lib.M_COHERENCE_MAGNITUDE)
    wide = (c_int * 1)(1)
    outs = (c_void_p * 1)(256)
    m = lib.sc_seed_measure_f64
    assert m(None, 5, fake, 2, None, 6, planes, 8, 1, one, wide, outs, None) == -1
    assert m(fake, 5, None, 2, None, 6, planes, 8, 1, one, wide, outs, None) == -1
    assert m(fake, 5, fake, 2, None, 6, planes, 8, 1, None, wide, outs, None) == -1
    assert m(fake, 5, fake, 2, None, 6, planes, 8, 1, one, wide, None, None) == -1
    assert m(fake, 0, fake, 2, None, 6, planes, 8, 1, one, wide, outs, None) == -1
    assert m(fake, 5, fake, 2, None, 6, planes, 0, 1, one, wide, outs, None) == -1
    assert m(fake, 5, fake, 65, None, 6, planes, 8, 1, one, wide, outs, None) == -1
    assert m(fake, 5, fake, 2, None, 6, planes, 8, 0, one, wide, outs, None) == -1
    assert m(fake, 5, fake, 2, None, 6, planes, 8, 11, one, wide, outs, None) == -1
    assert m(fake, 5, fake, 2, None, 6, _lib.PLANE_CSM, 8, 1, one, wide, outs, None) == -1          # coherence without the powers
    assert b"needs the planes" in lib.sc_last_error()
    assert m(fake, 5, fake, 2, None, 6, planes, 8, 1, (c_int * 1)(_lib.M_POWER), wide, outs, None) == -1
    assert b"not one of the ten" in lib.sc_last_error()
    assert m(fake, 5, fake, 2, None, 6, planes, 8, 1, one, wide, (c_void_p * 1)(None), None) == -1


def test_bad_requests_raise_before_any_device_work():
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(0)
    coef = rng.standard_normal((1, 3, 2, 8, 70)) + 1j * rng.standard_normal((1, 3, 2, 8, 70))
    c = sc.Connectivity(coef)
    for kwargs, match in ((dict(seeds=[0], measures=("coherence",)), "unknown measure"),
                          (dict(seeds=[0], measures=()), "measures is empty"),
                          (dict(seeds=[0], measures=("coherency", "coherency")), "twice"),
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
            c.seed_connectivity(**kwargs)
    assert c._spectra is None and not c._accum_cache           # nothing was uploaded or accumulated
    seeds, targets, names, codes, planes = _lib.seed_request((3, 1), None, "weighted_phase_lag_index", 8, 64)
    assert seeds.dtype == np.int32 and list(seeds) == [3, 1] and targets is None and names == ["weighted_phase_lag_index"]
    assert codes == [_lib.M_WPLI] and planes == _lib.PLANE_CSM | _lib.PLANE_ABS_IM
    *_, planes = _lib.seed_request([0], [2, 1], ("phase_lag_index", "coherency", "phase_locking_value"), 8, 64)
    assert planes == _lib.PLANE_SIGN_IM | _lib.PLANE_CSM | _lib.SEED_PLANE_POWER | _lib.PLANE_UNIT


def test_torch_free_host_refuses_more_than_256_signals():
    import subprocess
    import sys
    code = ("import sys\nimport numpy as np\nimport spectral_connectivity_amd as sc\n"
            "c = sc.Connectivity(np.ones((1, 2, 1, 8, 257), dtype=complex))\n"
            "try:\n    c.seed_connectivity([0])\nexcept ValueError as exc:\n    print('refused:', exc)\n"
            "assert 'torch' not in sys.modules\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, SC_HIP_HOST="numpy"))
    assert out.returncode == 0, out.stderr[-3000:]
    assert "refused:" in out.stdout and "more than 256 signals" in out.stdout, out.stdout


def test_wrapper_leaves_seed_connectivity_out():
    from spectral_connectivity_amd import wrapper
    assert "seed_connectivity" in wrapper._NOT_IN_DATASET
    with pytest.raises(ValueError, match="Connectivity class directly"):
        wrapper._check_method("seed_connectivity")
