"""CPU-only checks of the linear dependence boundary: sc_linear_dependence_f64 is declared in include/sc_hip.h with the argument
types of _lib.py's ctypes prototype and exported by libsc_hip.so (ABI version still 8), rejects NULL arguments, records without
the cross-spectral planes, three NULL outputs and pairs beyond sc_linear_dependence_max_joint() before any device work, the label
planning shared by both hosts (_lib.dependence_groups) checks labels and pair sizes, and both method names are in the wrapper's
lists.

The pair-size check of the entry point without a device: the group sizes are a DEVICE array, so here only what the scalar
arguments decide can be asked of it -- a group of 128 signals has no partner (the pair holds at least 129).  Groups of (2, 127)
signals are refused with the pair size where their sizes are known without a device: by _lib.dependence_groups, which both hosts
call before any device work (ValueError, "129").  The entry point's own SC_EUNSUPPORTED for (2, 127), from the sizes it reads back
before any launch, is asserted where there is a device: tests/test_gpu_linear_dependence.py::test_errors."""
import os
import re
from ctypes import POINTER, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sc_linear_dependence_f64"


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
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


def test_header_matches_the_ctypes_prototype():
    ret, args = declaration(NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert ret == "int" and restype is c_int
    # the MIC call with three outputs in the place of its two
    _, mic = declaration("sc_imaginary_interaction_f64")
    assert args[:9] == mic[:9] and args[-2:] == mic[-2:]
    assert args[9:12] == ["double* d_total", "double* d_instantaneous", "double* d_lagged"]
    assert len(args) == len(argtypes) == 14
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{NAME} argument {i} ({arg}) is {want.__name__} in _lib.py"
    ret, args = declaration("sc_linear_dependence_max_joint")
    assert ret == "int" and args == ["void"] and _lib.SYMBOLS["sc_linear_dependence_max_joint"] == (c_int, [])


def test_symbol_is_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    assert hasattr(lib, NAME) and lib.sc_linear_dependence_max_joint() == 128


def test_argument_checks_before_any_device_work():
    lib = _lib.load()
    fake = c_void_p(256)                 # never dereferenced: every check below returns before a copy or a launch
    call = lib.sc_linear_dependence_f64
    assert call(None, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, fake, fake, None) == -1
    assert b"NULL argument" in lib.sc_last_error()
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, None, fake, 2, 4, fake, fake, fake, fake, None) == -1
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, fake, None, 2, 4, fake, fake, fake, fake, None) == -1
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, fake, None, None) == -1
    assert b"NULL argument" in lib.sc_last_error()
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, None, None, None, fake, None) == -1      # SC_EINVAL
    assert b"no output requested" in lib.sc_last_error()
    assert call(fake, 4, 8, _lib.PLANE_ABS_IM, 10, fake, fake, 2, 4, fake, fake, fake, fake, None) == -1
    assert b"SC_PLANE_CSM" in lib.sc_last_error()
    assert call(fake, 0, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, fake, fake, None) == -1
    assert call(fake, 4, 8, _lib.PLANE_CSM, 0, fake, fake, 2, 4, fake, fake, fake, fake, None) == -1
    # a group of 128 signals and any partner: 129 or more (a single output is enough to get this far)
    assert call(fake, 4, 258, _lib.PLANE_CSM, 300, fake, fake, 2, 128, None, None, fake, fake, None) == -5  # SC_EUNSUPPORTED
    msg = lib.sc_last_error()
    assert b"129" in msg and b"linear dependence" in msg


def test_dependence_groups():
    labels, members, sizes, stride = _lib.dependence_groups(np.array(["b", "a", "c", "a", "c", "c", "b"]), 7, 128)
    assert list(labels) == ["a", "b", "c"] and stride == 16
    assert sizes.tolist() == [2, 2, 3] and members[:, :3].tolist() == [[1, 3, -1], [0, 6, -1], [2, 4, 5]]
    assert members.dtype == np.int32 and sizes.dtype == np.int32
    labels, members, sizes, stride = _lib.dependence_groups(None, 33, 128)
    assert np.array_equal(labels, np.arange(33)) and sizes.tolist() == [1] * 33 and stride == 16
    assert members[:, 0].tolist() == list(range(33)) and (members[:, 1:] == -1).all()
    # 300 single signals: no pair is large
    assert len(_lib.dependence_groups(None, 300, 128)[0]) == 300
    # (1, 127) and (64, 64) are the largest pairs
    assert _lib.dependence_groups([0] + [1] * 127, 128, 128)[2].tolist() == [1, 127]
    assert _lib.dependence_groups([0] * 64 + [1] * 64, 128, 128)[2].tolist() == [64, 64]


def test_dependence_groups_errors():
    with pytest.raises(ValueError, match="at least two groups"):
        _lib.dependence_groups([1, 1, 1], 3, 128)
    with pytest.raises(ValueError, match="one label per signal"):
        _lib.dependence_groups([0, 1], 3, 128)
    with pytest.raises(ValueError, match="at least two signals"):
        _lib.dependence_groups(None, 1, 128)
    with pytest.raises(ValueError, match=r"groups 'p' and 'q' have 129 signals together.*at most 128"):
        _lib.dependence_groups(["q"] * 127 + ["p"] * 2, 129, 128)
    # the two largest groups decide, wherever they stand
    with pytest.raises(ValueError, match=r"groups 0 and 2 have 130 signals together"):
        _lib.dependence_groups([0] * 65 + [1] * 3 + [2] * 65, 133, 128)
    with pytest.raises(ValueError, match="have 201 signals together"):
        _lib.dependence_groups([0] * 200 + [1], 201, 128)


def test_rank_rule_count():
    assert _lib.dependence_rank_skipped(np.array([2, 3, 4], np.int32), 5) == 2       # (2, 4) and (3, 4)
    assert _lib.dependence_rank_skipped(np.array([2, 3, 4], np.int32), 7) == 0
    assert _lib.dependence_rank_skipped(np.array([1] * 5, np.int32), 1) == 10


def test_wrapper_lists():
    from spectral_connectivity_amd import wrapper
    for name in ("linear_dependence", "lagged_coherence"):
        assert name in wrapper._NOT_IN_DATASET
    with pytest.raises(ValueError, match="Connectivity class directly"):
        wrapper._check_method("linear_dependence")
    wrapper._check_method("lagged_coherence")            # by name through multitaper_connectivity, as the partial coherences
    from spectral_connectivity_amd.connectivity import Connectivity, LinearDependence
    assert callable(Connectivity.linear_dependence) and callable(Connectivity.lagged_coherence)
    assert LinearDependence._fields == ("total", "instantaneous", "lagged", "labels")
