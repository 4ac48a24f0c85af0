"""CPU-only checks of the partial coherence boundary: sc_partial_coherence_max_signals / sc_partial_coherence_f64 are declared in
include/sc_hip.h with the argument types of _lib.py's ctypes prototypes and exported by libsc_hip.so, the ABI version has not
moved, every invalid argument is rejected with SC_EINVAL and a message before any device work, and the xarray wrapper keeps the
three measures out of its default Dataset."""
import os
import re
from ctypes import POINTER, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sc_partial_coherence_f64"
LIMIT = "sc_partial_coherence_max_signals"
SC_EINVAL = -1


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_hip.h")).read(), flags=re.S)


def declaration(name):
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header())
    assert m, f"{name} is not declared in sc_hip.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def ctype_of(arg):
    arg = re.sub(r"\bconst\b", "", arg).strip()
    if arg.startswith("int32_t*"):
        return (c_void_p, POINTER(c_int32))
    if "*" in arg:
        return (c_void_p,)
    base = arg.split()[0]
    return ({"int64_t": c_int64, "uint32_t": c_uint32, "double": c_double, "int": c_int, "size_t": c_size_t}[base],)


def test_header_matches_the_ctypes_prototypes():
    ret, args = declaration(LIMIT)
    assert ret == "int" and args == ["void"] and _lib.SYMBOLS[LIMIT] == (c_int, [])
    ret, args = declaration(NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert ret == "int" and restype is c_int
    # the head of the canonical coherence call (record, bins, signals, planes, observations), three outputs, then its tail
    _, canon = declaration("sc_canonical_coherence_f64")
    assert args[:5] == canon[:5] and args[-2:] == canon[-2:]
    assert args[5:8] == ["void* d_coherency", "double* d_magnitude", "double* d_multiple"]
    assert len(args) == len(argtypes) == 10
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{NAME} argument {i} ({arg}) is {want.__name__} in _lib.py"


def test_library_exports_both_symbols_and_keeps_the_abi_version():
    lib = _lib.load()
    assert callable(getattr(lib, NAME)) and callable(getattr(lib, LIMIT))
    assert lib.sc_partial_coherence_max_signals() == 128
    assert re.search(r"#define\s+SC_ABI_VERSION\s+8\b", header())
    assert lib.sc_abi_version() == 8


@pytest.mark.parametrize("what, change, message", [
    ("NULL record", dict(d_accum=None), b"NULL argument"),
    ("NULL fail counter", dict(d_fail=None), b"NULL argument"),
    ("no output", dict(d_coherency=None, d_magnitude=None, d_multiple=None), b"no output requested"),
    ("one signal", dict(n_signals=1), b"at least two signals"),
    ("129 signals", dict(n_signals=129), b"at most 128 signals (got 129)"),
    ("no CSM plane", dict(planes=_lib.PLANE_ABS_IM), b"SC_PLANE_CSM"),
    ("no bins", dict(n_bins=0), b"empty problem"),
    ("no observations", dict(n_observations=0), b"n_observations must be positive"),
])
def test_argument_checks_before_any_device_work(what, change, message):
    lib = _lib.load()
    fake = c_void_p(256)                 # never dereferenced: every check returns before a launch
    args = dict(d_accum=fake, n_bins=4, n_signals=8, planes=_lib.PLANE_CSM, n_observations=10, d_coherency=fake,
                d_magnitude=fake, d_multiple=fake, d_fail=fake, stream=None)
    args.update(change)
    assert lib.sc_partial_coherence_f64(*args.values()) == SC_EINVAL, what
    msg = lib.sc_last_error()
    assert msg.startswith(b"invalid argument") and message in msg, (what, msg)


def test_one_output_is_enough_for_the_argument_checks():
    """Any single output pointer passes the output check (the next check, the signal count, is what answers here)."""
    lib = _lib.load()
    fake = c_void_p(256)
    for outs in ((fake, None, None), (None, fake, None), (None, None, fake)):
        assert lib.sc_partial_coherence_f64(fake, 4, 129, _lib.PLANE_CSM, 10, *outs, fake, None) == SC_EINVAL
        assert b"at most 128 signals" in lib.sc_last_error()


def test_wrapper_keeps_the_measures_out_of_the_default_dataset():
    from spectral_connectivity_amd import wrapper
    from spectral_connectivity_amd.connectivity import Connectivity
    for name in ("partial_coherency", "partial_coherence_magnitude", "multiple_coherence_magnitude"):
        assert name in wrapper._NOT_IN_DATASET
        assert callable(getattr(Connectivity, name))
        wrapper._check_method(name)          # (an explicit request by name is served)
