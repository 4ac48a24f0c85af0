"""CPU-only checks of the multivariate imaginary coherence boundary: sc_imaginary_interaction_f64 is declared in
include/sc_hip.h with the argument types of _lib.py's ctypes prototype and exported by libsc_hip.so, rejects NULL arguments and
groups beyond sc_canonical_max_group() before any device work, the label planning shared by both hosts
(_lib.interaction_groups / member_table / interaction_kept) checks the labels, and the xarray wrapper leaves both measures out."""
import os
import re
from ctypes import POINTER, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sc_imaginary_interaction_f64"


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
    # the canonical coherence call with the one output split in two (MIC, MIM)
    _, canon = declaration("sc_canonical_coherence_f64")
    assert args[:9] == canon[:9] and args[-2:] == canon[-2:] and args[9:11] == ["double* d_mic", "double* d_mim"]
    assert len(args) == len(argtypes) == 13
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{NAME} argument {i} ({arg}) is {want.__name__} in _lib.py"


def test_argument_checks_before_any_device_work():
    lib = _lib.load()
    assert lib.sc_canonical_max_group() == 128
    fake = c_void_p(256)                 # never dereferenced: every check below returns before a launch
    call = lib.sc_imaginary_interaction_f64
    assert call(None, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, fake, None) == -1
    assert b"NULL argument" in lib.sc_last_error()
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, None, fake, None) == -1
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, None, fake, fake, None) == -1
    assert call(fake, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, None, None) == -1
    assert call(fake, 4, 8, _lib.PLANE_ABS_IM, 10, fake, fake, 2, 4, fake, fake, fake, None) == -1
    assert call(fake, 0, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, fake, None) == -1
    assert call(fake, 4, 258, _lib.PLANE_CSM, 10, fake, fake, 2, 129, fake, fake, fake, None) == -5     # SC_EUNSUPPORTED
    msg = lib.sc_last_error()
    assert b"129" in msg and b"imaginary interaction" in msg


def test_interaction_groups():
    labels, members, sizes, stride = _lib.interaction_groups(np.array(["b", "a", "c", "a", "c", "c", "b"]), 7, 128)
    assert list(labels) == ["a", "b", "c"] and stride == 16
    assert sizes.tolist() == [2, 2, 3] and members.shape == (3, 16)
    assert members[:, :3].tolist() == [[1, 3, -1], [0, 6, -1], [2, 4, 5]] and (members[:, 3:] == -1).all()
    assert members.dtype == np.int32 and sizes.dtype == np.int32
    for size, want in ((16, 16), (17, 32), (32, 32), (33, 128), (128, 128)):
        _, members, sizes, stride = _lib.interaction_groups(np.r_[np.zeros(size, int), 1], size + 1, 128)
        assert stride == want and members.shape == (2, want) and sizes.tolist() == [size, 1]
    # the table of a subset (the groups the rank rule keeps) has the stride of ITS largest group
    members, sizes, stride = _lib.member_table([np.arange(40), np.arange(40, 43)])
    sub, sub_sizes, sub_stride = _lib.member_table([members[1, :sizes[1]]])
    assert stride == 128 and sub_stride == 16 and sub[0, :3].tolist() == [40, 41, 42]


def test_interaction_kept():
    keep, n_out = _lib.interaction_kept(np.array([3, 9, 8, 1], np.int32), 4)
    assert keep.tolist() == [0, 2, 3] and n_out == 1


def test_interaction_groups_errors():
    with pytest.raises(ValueError, match="at least two groups"):
        _lib.interaction_groups([1, 1, 1], 3, 128)
    with pytest.raises(ValueError, match="one label per signal"):
        _lib.interaction_groups([0, 1], 3, 128)
    with pytest.raises(ValueError, match="group 'x' has 129 channels"):
        _lib.interaction_groups(["x"] * 129 + ["y"] * 3, 132, 128)


def test_wrapper_leaves_both_measures_out():
    from spectral_connectivity_amd import wrapper
    for name in ("maximized_imaginary_coherence", "multivariate_interaction_measure"):
        assert name in wrapper._NOT_IN_DATASET
        with pytest.raises(ValueError, match="Connectivity class directly"):
            wrapper._check_method(name)
    from spectral_connectivity_amd.connectivity import Connectivity
    assert callable(Connectivity.maximized_imaginary_coherence) and callable(Connectivity.multivariate_interaction_measure)
