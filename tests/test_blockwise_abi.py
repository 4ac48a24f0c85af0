"""CPU-only checks of the blockwise Granger boundary (ABI v8): the two entry points are declared in include/sc_hip.h with the
argument types of _lib.py's ctypes prototypes, exported by libsc_hip.so, the workspace query enforces the pair-size limit, and
the host planning shared by both hosts (_lib.blockwise_pairs / blockwise_batches) rejects bad labels and batches the block pairs."""
import os
import re
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_blockwise_granger_workspace_bytes", "sc_blockwise_granger_f64")


def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sc_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in sc_hip.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def ctype_of(arg):
    arg = re.sub(r"\bconst\b", "", arg).strip()
    if arg.startswith("int32_t*"):
        return (c_void_p, POINTER(c_int32))
    if arg.startswith("size_t*"):
        return (POINTER(c_size_t),)
    if "*" in arg:
        return (c_void_p,)
    base = arg.split()[0]
    return ({"int64_t": c_int64, "uint32_t": c_uint32, "double": c_double, "int": c_int, "size_t": c_size_t}[base],)


def test_header_matches_the_ctypes_prototypes():
    assert _lib.SC_ABI_VERSION == 8
    assert re.search(r"#define SC_ABI_VERSION 8\b", open(os.path.join(ROOT, "include", "sc_hip.h")).read())
    for name in NAMES:
        ret, args = declaration(name)
        restype, argtypes = _lib.SYMBOLS[name]
        assert ret == "int" and restype is c_int
        assert len(args) == len(argtypes), name
        for i, (arg, want) in enumerate(zip(args, argtypes)):
            assert want in ctype_of(arg), f"{name} argument {i} ({arg}) is {want.__name__} in _lib.py"


def test_exported_and_workspace_limits():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    nbytes = c_size_t()
    assert lib.sc_blockwise_granger_workspace_bytes(7, 32, 256, 28, byref(nbytes)) == 0
    small = nbytes.value
    # the pair spectra and factors alone: two complex128 arrays [pairs x groups][N][m][m]
    assert small >= 2 * 7 * 28 * 256 * 32 * 32 * 16
    assert lib.sc_blockwise_granger_workspace_bytes(7, 32, 256, 56, byref(nbytes)) == 0 and nbytes.value > small
    assert lib.sc_blockwise_granger_workspace_bytes(1, 512, 64, 1, byref(nbytes)) == 0
    assert lib.sc_blockwise_granger_workspace_bytes(1, 513, 64, 1, byref(nbytes)) == -5        # SC_EUNSUPPORTED
    assert b"513" in lib.sc_last_error()
    assert lib.sc_blockwise_granger_workspace_bytes(1, 1, 64, 1, byref(nbytes)) == -5
    # argument checks before any device work
    assert lib.sc_blockwise_granger_f64(None, None, 1, 64, 64, 4, _lib.PLANE_CSM, 8, None, None, None, 1, 4, 2, 1e-8, 60,
                                        None, 0, 0, None, None, None, None, None) == -1


def test_blockwise_pairs_and_batches():
    labels, pairs = _lib.blockwise_pairs(np.array(["b", "a", "c", "a", "c", "c", "b"]), 7, 512)
    assert list(labels) == ["a", "b", "c"]
    batches, skipped = _lib.blockwise_batches(pairs, n_obs=100)
    assert skipped == 0
    # pairs (a, b): m = 4, (a, c): 5, (b, c): 5 -- batched by m, signals of the first block first
    assert sorted(batches) == [4, 5]
    members, split, cell = batches[4]
    assert members.tolist() == [[1, 3, 0, 6]] and split.tolist() == [2] and cell.tolist() == [[0, 1]]
    members, split, cell = batches[5]
    assert members.tolist() == [[1, 3, 2, 4, 5], [0, 6, 2, 4, 5]] and split.tolist() == [2, 2]
    assert cell.tolist() == [[0, 2], [1, 2]]
    assert all(a.dtype == np.int32 for batch in batches.values() for a in batch)
    # a pair of more signals than observations is left out (rank-deficient spectrum)
    _, pairs = _lib.blockwise_pairs([0, 0, 0, 1, 2], 5, 512)
    batches, skipped = _lib.blockwise_batches(pairs, n_obs=3)
    assert skipped == 2 and list(batches) == [2]


def test_blockwise_pairs_errors():
    with pytest.raises(ValueError, match="at least two groups"):
        _lib.blockwise_pairs([1, 1, 1], 3, 512)
    with pytest.raises(ValueError, match="one label per signal"):
        _lib.blockwise_pairs([0, 1], 3, 512)
    with pytest.raises(ValueError, match=r"groups 0 and 1 have 513 signals"):
        _lib.blockwise_pairs([0] * 300 + [1] * 213 + [2] * 5, 518, 512)
