"""CPU-only checks of the jackknife boundary: the entry points of sc_jackknife.hip are declared in include/sc_hip.h with the
argument types of _lib.py's ctypes prototypes and exported by libsc_hip.so, SC_ABI_VERSION is still 8, the layout query and the
argument checks answer without a device, and the request planning shared by both hosts checks its arguments."""
import os
import re
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_jackknife_layout", "sc_jackknife_workspace_bytes", "sc_jackknife_f32", "sc_jackknife_f64")


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_hip.h")).read(), flags=re.S)


def declaration(name):
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, f"{name} is not declared in sc_hip.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def ctype_of(arg):
    arg = re.sub(r"\bconst\b", "", arg).strip()
    if arg.startswith("sc_spectra_desc*"):
        return (POINTER(_lib.SpectraDesc),)
    if arg.startswith("int64_t*"):
        return (POINTER(c_int64),)
    if arg.startswith("int32_t*"):
        return (c_void_p, POINTER(c_int32))
    if "*" in arg:
        return (c_void_p,)
    base = arg.split()[0]
    return ({"int64_t": c_int64, "uint32_t": c_uint32, "double": c_double, "int": c_int, "size_t": c_size_t}[base],)


@pytest.mark.parametrize("name", NAMES)
def test_header_matches_the_ctypes_prototype(name):
    ret, args = declaration(name)
    restype, argtypes = _lib.SYMBOLS[name]
    assert {"int": c_int, "int64_t": c_int64}[ret] is restype
    assert len(args) == len(argtypes) == {"sc_jackknife_layout": 7, "sc_jackknife_workspace_bytes": 5}.get(name, 13)
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{name} argument {i} ({arg}) is {want.__name__} in _lib.py"
    assert declaration("sc_jackknife_f32")[1][1:] == declaration("sc_jackknife_f64")[1][1:]


def test_abi_version_and_constants():
    assert re.search(r"#define\s+SC_ABI_VERSION\s+8\b", header()) and _lib.SC_ABI_VERSION == 8
    text = header()
    for name, (bit, _, _) in _lib.JACKKNIFE_MEASURES.items():
        assert re.search(r"#define\s+SC_JACKKNIFE_" + name.upper() + r"\s+" + hex(bit) + "u", text), name
    for name, code in _lib.JACKKNIFE_OVER.items():
        assert re.search(r"#define\s+SC_JACKKNIFE_OVER_" + name.upper() + r"\s+" + str(code) + r"\b", text), name
    assert "sc_jackknife.hip" in _lib._build.SOURCES and os.path.exists(os.path.join(_lib._build.CSRC, "sc_jackknife.hip"))


def desc(F=5, W=3, R=4, K=2, C=6, reduce=(0, 1, 1)):
    return _lib.SpectraDesc(n_freq=F, n_windows=W, n_trials=R, n_tapers=K, n_signals=C, stride_freq=W * R * K * C,
                            stride_window=R * K * C, stride_trial=K * C, stride_taper=C, reduce_window=reduce[0],
                            reduce_trial=reduce[1], reduce_taper=reduce[2], reserved=0)


def test_library_exports_and_answers_without_a_device():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    for name in NAMES:
        assert hasattr(lib, name)
    n_bins, n_units, unit, n_out = c_int64(), c_int64(), c_int64(), c_int64()
    d = desc()
    assert lib.sc_jackknife_layout(byref(d), 0x7, 0, byref(n_bins), byref(n_units), byref(unit), byref(n_out)) == 0
    assert (n_bins.value, n_units.value, unit.value) == (15, 4, 2)
    assert n_out.value == 3 * 15 * (6 + 36 + 36)
    assert lib.sc_jackknife_layout(byref(d), 0x2, 1, byref(n_bins), byref(n_units), byref(unit), byref(n_out)) == 0
    assert (n_units.value, unit.value, n_out.value) == (8, 1, 3 * 15 * 36)
    d = desc(reduce=(1, 1, 1))
    assert lib.sc_jackknife_layout(byref(d), 0x1, 0, byref(n_bins), byref(n_units), byref(unit), byref(n_out)) == 0
    assert (n_bins.value, n_units.value, unit.value, n_out.value) == (5, 4, 6, 3 * 5 * 6)
    # a kept trial axis has no trial units; an empty or unknown mask; a bad `over`
    assert lib.sc_jackknife_layout(byref(desc(reduce=(0, 0, 1))), 0x2, 0, None, None, None, None) == -1
    assert b"averages over trials" in lib.sc_last_error()
    assert lib.sc_jackknife_layout(byref(d), 0, 0, None, None, None, None) == -1
    assert lib.sc_jackknife_layout(byref(d), 0x8, 0, None, None, None, None) == -1
    assert lib.sc_jackknife_layout(byref(d), 0x2, 2, None, None, None, None) == -1
    # few (bin, tile pair) workgroups and many units: the units are split, the workspace holds one output per split
    many = desc(F=1, W=1, R=640, K=1, C=4, reduce=(0, 1, 1))
    lib.sc_jackknife_layout(byref(many), 0x2, 0, None, None, None, byref(n_out))
    ws = lib.sc_jackknife_workspace_bytes(byref(many), 0x2, 0, 0, 640)
    assert ws == 40 * n_out.value * 8
    assert lib.sc_jackknife_workspace_bytes(byref(desc(F=600, C=64)), 0x2, 0, 0, 4) == 0
    fake = c_void_p(256)                 # never dereferenced: every check below returns before a launch
    for fn in (lib.sc_jackknife_f32, lib.sc_jackknife_f64):
        assert fn(None, byref(d), fake, _lib.PLANE_CSM, 0x2, 0, 0, 4, 4, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, _lib.PLANE_ABS_IM, 0x2, 0, 0, 4, 4, fake, None, 0, None) == -1
        assert fn(fake, byref(d), fake, _lib.PLANE_CSM, 0x2, 0, 0, 5, 5, fake, None, 0, None) == -1      # units beyond the spectra's
        assert fn(fake, byref(d), fake, _lib.PLANE_CSM, 0x2, 0, 0, 1, 1, fake, None, 0, None) == -1      # fewer than two units in all
        assert b"at least two units" in lib.sc_last_error()
        assert fn(fake, byref(many), fake, _lib.PLANE_CSM, 0x2, 0, 0, 640, 640, fake, None, 0, None) == -1
        assert b"workspace too small" in lib.sc_last_error()


def test_request_planning():
    names, mask, over, n = _lib.jackknife_request(("imaginary_coherence", "power"), "trials", "trials_tapers", 5, 35)
    assert names == ["power", "imaginary_coherence"] and mask == 0x5 and over == 0 and n == 5
    names, mask, over, n = _lib.jackknife_request("coherence_magnitude", "observations", "tapers", 1, 7)
    assert names == ["coherence_magnitude"] and mask == 0x2 and over == 1 and n == 7
    blocks, total = _lib.jackknife_blocks(["power", "imaginary_coherence"], 10, 3)
    assert blocks == [("power", 0, 30, (10, 3)), ("imaginary_coherence", 90, 90, (10, 3, 3))] and total == 360
    for args, match in (((("coherence",), "trials", "trials_tapers", 5, 35), "unknown measure"),
                        (((), "trials", "trials_tapers", 5, 35), "empty"),
                        ((("power",), "units", "trials_tapers", 5, 35), "over must be"),
                        ((("power",), "trials", "time_tapers", 5, 35), "averages over trials"),
                        ((("power",), "trials", "trials", 1, 1), "n_trials >= 2"),
                        ((("power",), "observations", "tapers", 9, 1), "n_observations >= 2")):
        with pytest.raises(ValueError, match=match):
            _lib.jackknife_request(*args)


def test_wrapper_leaves_the_jackknife_out():
    from spectral_connectivity_amd import wrapper
    assert "jackknife" in wrapper._NOT_IN_DATASET
    with pytest.raises(ValueError, match="Connectivity class directly"):
        wrapper._check_method("jackknife")
