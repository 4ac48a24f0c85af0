"""CPU-only checks of the canonical-coherence vectors boundary: sc_canonical_coherence_vectors_f64 and
sc_canonical_vectors_lds_group are declared in include/sc_hip.h with the argument types of _lib.py's ctypes prototypes and exported
by libsc_hip.so (ABI version still 8), the entry point rejects NULL arguments and groups of more than 128 channels before any device
work, the LDS edge is where tests/canonical_vectors_ref.py puts it, and the method name is in the wrapper's lists."""
from ctypes import c_int, c_void_p

import pytest

import canonical_vectors_ref as cvref
from spectral_connectivity_amd import _lib
from test_linear_dependence_abi import ctype_of, declaration

NAME = "sc_canonical_coherence_vectors_f64"


def test_header_matches_the_ctypes_prototype():
    ret, args = declaration(NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert ret == "int" and restype is c_int
    # the MIC vectors call with four outputs in the place of its three
    _, mic = declaration("sc_imaginary_interaction_vectors_f64")
    assert args[:9] == mic[:9] and args[-2:] == mic[-2:]
    assert args[9:13] == ["double* d_coherence", "double* d_coherences", "double* d_filters", "double* d_patterns"]
    assert len(args) == len(argtypes) == 15
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{NAME} argument {i} ({arg}) is {want.__name__} in _lib.py"
    ret, args = declaration("sc_canonical_vectors_lds_group")
    assert ret == "int" and args == ["int max_group_size"] and _lib.SYMBOLS["sc_canonical_vectors_lds_group"] == (c_int, [c_int])


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    assert hasattr(lib, NAME) and hasattr(lib, "sc_canonical_vectors_lds_group") and lib.sc_canonical_max_group() == 128


def test_argument_checks_before_any_device_work():
    lib = _lib.load()
    fake = c_void_p(256)                 # never dereferenced: every check below returns before a copy or a launch
    call = getattr(lib, NAME)
    good = [fake, 4, 8, _lib.PLANE_CSM, 10, fake, fake, 2, 4, fake, fake, fake, fake, fake, None]
    for k in (0, 5, 6, 9, 10, 11, 12, 13):
        args = list(good)
        args[k] = None
        assert call(*args) == -1, k
        assert b"NULL argument" in lib.sc_last_error(), k
    args = list(good)
    args[3] = _lib.PLANE_ABS_IM
    assert call(*args) == -1 and b"SC_PLANE_CSM" in lib.sc_last_error()
    args = list(good)
    args[1] = 0
    assert call(*args) == -1
    args = list(good)
    args[8] = 0
    assert call(*args) == -1 and b"empty groups" in lib.sc_last_error()
    args = list(good)
    args[2], args[4], args[8] = 258, 300, 129
    assert call(*args) == -5                                                   # SC_EUNSUPPORTED
    msg = lib.sc_last_error()
    assert b"128" in msg and b"canonical coherence vectors" in msg


def test_lds_edge_is_where_the_size_cases_put_it():
    """A layout change cannot move the edge silently: the reference module hard-codes it."""
    lib = _lib.load()
    e = cvref.LDS_EDGE
    assert e == 51
    assert lib.sc_canonical_vectors_lds_group(e) == e and lib.sc_canonical_vectors_lds_group(e + 1) <= e
    assert (e, e) in cvref.GROUP_SIZES and (e, e + 1) in cvref.GROUP_SIZES
    assert lib.sc_canonical_vectors_lds_group(129) == 0 and lib.sc_canonical_vectors_lds_group(128) >= 1
    assert lib.sc_canonical_vectors_lds_group(0) == 0
    # the complex vectors take 4 KB more than the real ones: never more room than the MIC vectors have
    for n in range(1, 129):
        assert 1 <= lib.sc_canonical_vectors_lds_group(n) <= lib.sc_interaction_vectors_lds_group(n)


def test_wrapper_lists_and_the_named_tuple():
    from spectral_connectivity_amd import wrapper
    assert "canonical_coherence_vectors" in wrapper._NOT_IN_DATASET
    with pytest.raises(ValueError, match="Connectivity class directly"):
        wrapper._check_method("canonical_coherence_vectors")
    from spectral_connectivity_amd.connectivity import CanonicalVectors, Connectivity
    assert callable(Connectivity.canonical_coherence_vectors)
    assert CanonicalVectors._fields == ("coherence", "coherences", "filters", "patterns", "labels", "members")
    doc = Connectivity.canonical_coherence_vectors.__doc__
    assert "not distinguishable from 0" in doc and "nearly coincide" in doc
