"""CPU-only checks of the boundary of partial coherence given a chosen set: the five entry points are declared in include/sc_hip.h
with the argument types of _lib.py's ctypes prototypes and exported by libsc_hip.so, the ABI version has not moved, the LDS query
is the documented formula, and every invalid argument is rejected with SC_EINVAL and a message before any device work."""
import inspect
import re
from ctypes import c_int, c_int64, c_void_p

import pytest

from spectral_connectivity_amd import _lib
from test_partial_coherence_abi import ctype_of, declaration, header

NAME = "sc_partial_coherence_given_f64"
SC_EINVAL = -1


def lds_bytes(a, m):
    return (m * (m + 1) // 2 + m * a) * 16 + (2 * a + m) * 8 + 16


def test_header_matches_the_ctypes_prototypes():
    for name in ("sc_partial_given_max_given", "sc_partial_given_max_kept"):
        assert declaration(name) == ("int", ["void"]) and _lib.SYMBOLS[name] == (c_int, [])
    assert declaration("sc_partial_given_lds_limit") == ("int64_t", ["void"])
    assert _lib.SYMBOLS["sc_partial_given_lds_limit"] == (c_int64, [])
    assert declaration("sc_partial_given_lds_bytes") == ("int64_t", ["int64_t n_kept", "int64_t n_given"])
    assert _lib.SYMBOLS["sc_partial_given_lds_bytes"] == (c_int64, [c_int64, c_int64])
    ret, args = declaration(NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert ret == "int" and restype is c_int
    _, full = declaration("sc_partial_coherence_f64")
    assert args[:5] == full[:5] and args[-2:] == full[-2:]                 # the record head and the (fail, stream) tail
    assert args[5:9] == ["const int32_t* d_kept", "int n_kept", "const int32_t* d_given", "int n_given"]
    assert args[9:12] == ["void* d_coherency", "double* d_magnitude", "double* d_multiple"]
    assert len(args) == len(argtypes) == 14
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{NAME} argument {i} ({arg}) is {want.__name__} in _lib.py"


def test_library_exports_the_symbols_and_keeps_the_abi_version():
    lib = _lib.load()
    assert callable(getattr(lib, NAME))
    assert lib.sc_partial_given_max_given() == 128 and lib.sc_partial_given_max_kept() == 1024
    assert lib.sc_partial_given_lds_limit() == 160 * 1024
    assert re.search(r"#define\s+SC_ABI_VERSION\s+8\b", header())
    assert lib.sc_abi_version() == 8


def test_lds_query_is_the_documented_formula():
    lib = _lib.load()
    limit = lib.sc_partial_given_lds_limit()
    for a, m in ((1, 1), (3, 4), (300, 6), (1024, 8), (512, 16), (14, 128), (15, 128), (192, 128), (1024, 128)):
        assert lib.sc_partial_given_lds_bytes(a, m) == lds_bytes(a, m)
    for a, m in ((0, 1), (1, 0), (1025, 1), (1, 129), (-1, 4)):
        assert lib.sc_partial_given_lds_bytes(a, m) == -1
    # what the header advertises fits, the next size does not
    assert all(lds_bytes(a, m) <= limit for a, m in ((1024, 8), (512, 16), (300, 6)))
    for a, m in ((14, 128), (559, 17)):
        assert lds_bytes(a, m) <= limit < lds_bytes(a + 1, m)
    assert all(lds_bytes(128 - m, m) <= limit for m in range(1, 128))
    assert lds_bytes(192, 128) > limit


@pytest.mark.parametrize("what, change, message", [
    ("NULL record", dict(d_accum=None), b"NULL argument"),
    ("NULL fail counters", dict(d_fail=None), b"NULL argument"),
    ("NULL kept list", dict(d_kept=None), b"NULL argument"),
    ("NULL given list", dict(d_given=None), b"NULL argument"),
    ("no output", dict(d_coherency=None, d_magnitude=None, d_multiple=None), b"no output requested"),
    ("no given signal", dict(n_given=0), b"(got 0 given, 3 kept)"),
    ("129 given signals", dict(n_given=129, n_signals=400), b"1 ... 128 given"),
    ("no kept signal", dict(n_kept=0), b"(got 2 given, 0 kept)"),
    ("1025 kept signals", dict(n_kept=1025, n_signals=2000), b"1 ... 1024 kept"),
    ("more than the record holds", dict(n_kept=7), b"out of the 8 of the record"),
    ("beyond the LDS", dict(n_kept=192, n_given=128, n_signals=320), b"192 kept signals given 128 need 529424 bytes"),
    ("no CSM plane", dict(planes=_lib.PLANE_ABS_IM), b"SC_PLANE_CSM"),
    ("no bins", dict(n_bins=0), b"empty problem"),
    ("no observations", dict(n_observations=0), b"n_observations must be positive"),
])
def test_argument_checks_before_any_device_work(what, change, message):
    lib = _lib.load()
    fake = c_void_p(256)                 # never dereferenced: every check returns before a launch
    args = dict(d_accum=fake, n_bins=4, n_signals=8, planes=_lib.PLANE_CSM, n_observations=10, d_kept=fake, n_kept=3, d_given=fake,
                n_given=2, d_coherency=fake, d_magnitude=fake, d_multiple=fake, d_fail=fake, stream=None)
    args.update(change)
    assert lib.sc_partial_coherence_given_f64(*args.values()) == SC_EINVAL, what
    msg = lib.sc_last_error()
    assert msg.startswith(b"invalid argument") and message in msg, (what, msg)


def test_public_methods_take_the_two_keywords():
    from spectral_connectivity_amd.connectivity import Connectivity
    for name in ("partial_coherency", "partial_coherence_magnitude", "multiple_coherence_magnitude"):
        params = inspect.signature(getattr(Connectivity, name)).parameters
        assert list(params) == ["self", "given", "signals"]
        assert params["given"].default is None and params["signals"].default is None
