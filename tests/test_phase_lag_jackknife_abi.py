"""CPU-only checks of the phase-lag jackknife boundary: the four sc_jackknife_phase_* entry points are declared in include/sc_hip.h
with the argument types of _lib.py's ctypes prototypes and exported by libsc_hip.so, SC_ABI_VERSION is still 8, the layout query and
every argument check answer without a device, the request planning shared by both hosts checks its arguments, and
statistics.jackknife_difference."""
import os
import re
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest
import scipy.stats

from spectral_connectivity_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_jackknife_phase_layout", "sc_jackknife_phase_workspace_bytes", "sc_jackknife_phase_f32", "sc_jackknife_phase_f64")
COUNTERPART = {name: name.replace("_phase", "") for name in NAMES}
PLI, WPLI, DPLI2, DWPLI2 = 0x1, 0x2, 0x4, 0x8


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
    for i, (arg, want) in enumerate(zip(args, argtypes)):
        assert want in ctype_of(arg), f"{name} argument {i} ({arg}) is {want.__name__} in _lib.py"
    # the same argument list as its counterpart of the first jackknife family
    assert (ret, args) == declaration(COUNTERPART[name])
    assert (restype, argtypes) == _lib.SYMBOLS[COUNTERPART[name]]


def test_abi_version_and_constants():
    text = header()
    assert re.search(r"#define\s+SC_ABI_VERSION\s+8\b", text) and _lib.SC_ABI_VERSION == 8
    short = {"phase_lag_index": "PLI", "weighted_phase_lag_index": "WPLI", "debiased_squared_phase_lag_index": "DEBIASED_PLI2",
             "debiased_squared_weighted_phase_lag_index": "DEBIASED_WPLI2"}
    assert list(_lib.JACKKNIFE_PHASE_MEASURES) == list(short)                   # (dict order = block order)
    for (name, (bit, transform, rank)), want in zip(_lib.JACKKNIFE_PHASE_MEASURES.items(), (PLI, WPLI, DPLI2, DWPLI2)):
        assert (bit, transform, rank) == (want, "identity", 2)
        assert re.search(r"#define\s+SC_JACKKNIFE_PHASE_" + short[name] + r"\s+" + hex(bit) + "u", text), name
    # the first family is not widened
    assert list(_lib.JACKKNIFE_MEASURES) == ["power", "coherence_magnitude", "imaginary_coherence"]


def desc(F=5, W=3, R=4, K=2, C=6, reduce=(0, 1, 1)):
    return _lib.SpectraDesc(n_freq=F, n_windows=W, n_trials=R, n_tapers=K, n_signals=C, stride_freq=W * R * K * C,
                            stride_window=R * K * C, stride_trial=K * C, stride_taper=C, reduce_window=reduce[0],
                            reduce_trial=reduce[1], reduce_taper=reduce[2], reserved=0)


def test_library_exports_and_layout():
    lib = _lib.load()
    assert lib.sc_abi_version() == 8
    for name in NAMES:
        assert hasattr(lib, name)
    n_bins, n_units, unit, n_out = c_int64(), c_int64(), c_int64(), c_int64()
    d = desc()
    assert lib.sc_jackknife_phase_layout(byref(d), 0xF, 0, byref(n_bins), byref(n_units), byref(unit), byref(n_out)) == 0
    assert (n_bins.value, n_units.value, unit.value, n_out.value) == (15, 4, 2, 4 * 3 * 15 * 36)
    d2 = desc(F=3, W=2, R=5, K=3, C=7, reduce=(1, 1, 1))
    assert lib.sc_jackknife_phase_layout(byref(d2), PLI | DWPLI2, 1, byref(n_bins), byref(n_units), byref(unit), byref(n_out)) == 0
    assert (n_bins.value, n_units.value, unit.value, n_out.value) == (3, 30, 1, 2 * 3 * 3 * 49)
    assert lib.sc_jackknife_phase_layout(byref(d2), PLI, 0, byref(n_bins), byref(n_units), byref(unit), byref(n_out)) == 0
    assert (n_units.value, unit.value) == (5, 6)
    # the first family's layout still refuses the bit it does not have
    assert lib.sc_jackknife_layout(byref(d), 0x8, 0, None, None, None, None) == -1
    # few (bin, tile pair) workgroups and many units: the units are split, the workspace holds one output per split
    many = desc(F=1, W=1, R=640, K=1, C=4, reduce=(0, 1, 1))
    lib.sc_jackknife_phase_layout(byref(many), 0xF, 0, None, None, None, byref(n_out))
    assert lib.sc_jackknife_phase_workspace_bytes(byref(many), 0xF, 0, 0, 640) == 40 * n_out.value * 8
    assert lib.sc_jackknife_phase_workspace_bytes(byref(desc(F=600, C=64)), WPLI, 0, 0, 4) == 0


def test_every_bad_argument_answers_without_a_device():
    lib = _lib.load()
    d = desc()
    all_planes = _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ | _lib.PLANE_SIGN_IM
    many = desc(F=1, W=1, R=640, K=1, C=4, reduce=(0, 1, 1))
    # layout: an empty mask, an unknown mask, a bad `over`, a kept trial axis under over = trials
    assert lib.sc_jackknife_phase_layout(byref(d), 0, 0, None, None, None, None) == -1
    assert b"non-empty mask" in lib.sc_last_error()
    assert lib.sc_jackknife_phase_layout(byref(d), 0x10, 0, None, None, None, None) == -1
    assert lib.sc_jackknife_phase_layout(byref(d), WPLI, 2, None, None, None, None) == -1
    assert b"over" in lib.sc_last_error()
    assert lib.sc_jackknife_phase_layout(byref(desc(reduce=(0, 0, 1))), WPLI, 0, None, None, None, None) == -1
    assert b"averages over trials" in lib.sc_last_error()
    assert lib.sc_jackknife_phase_layout(None, WPLI, 0, None, None, None, None) == -1
    fake = c_void_p(256)                 # never dereferenced: every check below returns before a launch
    for fn in (lib.sc_jackknife_phase_f32, lib.sc_jackknife_phase_f64):
        def call(X=fake, dd=d, total=fake, planes=all_planes, mask=WPLI, over=0, lo=0, hi=4, n=4, out=fake, ws=None, ws_bytes=0):
            return fn(X, byref(dd), total, planes, mask, over, lo, hi, n, out, ws, ws_bytes, None)
        assert call(mask=0) == -1 and b"non-empty mask" in lib.sc_last_error()
        assert call(mask=0x10) == -1
        assert call(over=2) == -1
        assert call(dd=desc(reduce=(0, 0, 1))) == -1 and b"averages over trials" in lib.sc_last_error()
        for null in ("X", "total", "out"):
            assert call(**{null: None}) == -1 and b"NULL argument" in lib.sc_last_error(), null
        assert call(hi=5, n=5) == -1 and b"unit range" in lib.sc_last_error()          # units beyond the spectra's
        assert call(lo=2, hi=2) == -1 and b"unit range" in lib.sc_last_error()
        assert call(hi=1, n=1) == -1 and b"at least two units" in lib.sc_last_error()   # fewer than two units in all
        assert call(dd=many, hi=640, n=640) == -1 and b"workspace too small" in lib.sc_last_error()
        assert call(dd=many, hi=640, n=640, ws=fake, ws_bytes=8) == -1 and b"workspace too small" in lib.sc_last_error()
        # a record that lacks a plane a requested measure reads
        for mask, needs in ((PLI, _lib.PLANE_SIGN_IM), (DPLI2, _lib.PLANE_SIGN_IM), (WPLI, _lib.PLANE_CSM | _lib.PLANE_ABS_IM),
                            (DWPLI2, _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ)):
            bit = 1
            while bit <= needs:
                if needs & bit:
                    assert call(mask=mask, planes=all_planes & ~bit) == -1, (mask, bit)
                    assert b"lacks a plane" in lib.sc_last_error(), (mask, bit)
                    assert call(mask=0xF, planes=all_planes & ~bit) == -1, (mask, bit)
                bit <<= 1
        # two units of one observation each: no debiased estimate of a delete-one set
        two = desc(F=3, W=1, R=2, K=1, C=3, reduce=(0, 1, 1))
        assert call(dd=two, mask=DPLI2, hi=2, n=2) == -1 and b"at least two observations" in lib.sc_last_error()
        assert call(dd=two, mask=DWPLI2, hi=2, n=2) == -1 and b"at least two observations" in lib.sc_last_error()


def test_totals_entry_points():
    """The record of totals the hosts hand to sc_jackknife_phase_*: declared as typed, exported, checked without a device."""
    lib = _lib.load()
    for name, n_args in (("sc_jackknife_phase_totals_workspace_bytes", 5), ("sc_jackknife_phase_totals_f32", 10),
                         ("sc_jackknife_phase_totals_f64", 10)):
        ret, args = declaration(name)
        restype, argtypes = _lib.SYMBOLS[name]
        assert {"int": c_int, "int64_t": c_int64}[ret] is restype and len(args) == len(argtypes) == n_args
        for i, (arg, want) in enumerate(zip(args, argtypes)):
            assert want in ctype_of(arg), f"{name} argument {i} ({arg}) is {want.__name__} in _lib.py"
        assert hasattr(lib, name)
    d, fake = desc(), c_void_p(256)
    sign, all_planes = _lib.PLANE_SIGN_IM, _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ | _lib.PLANE_SIGN_IM
    many = desc(F=1, W=1, R=640, K=1, C=4, reduce=(0, 1, 1))
    # 40 splits of one bin record: planes x one 16 x 16 tile of doubles
    assert lib.sc_jackknife_phase_totals_workspace_bytes(byref(many), sign, 0, 0, 640) == 40 * 1 * 256 * 8
    assert lib.sc_jackknife_phase_totals_workspace_bytes(byref(many), all_planes, 0, 0, 640) == 40 * 5 * 256 * 8
    assert lib.sc_jackknife_phase_totals_workspace_bytes(byref(desc(F=600, C=64)), sign, 0, 0, 4) == 0
    for fn in (lib.sc_jackknife_phase_totals_f32, lib.sc_jackknife_phase_totals_f64):
        assert fn(None, byref(d), sign, 0, 0, 4, fake, None, 0, None) == -1 and b"NULL argument" in lib.sc_last_error()
        assert fn(fake, byref(d), sign, 0, 0, 4, None, None, 0, None) == -1 and b"NULL argument" in lib.sc_last_error()
        assert fn(fake, byref(d), 0, 0, 0, 4, fake, None, 0, None) == -1 and b"planes" in lib.sc_last_error()
        assert fn(fake, byref(d), _lib.PLANE_UNIT, 0, 0, 4, fake, None, 0, None) == -1 and b"planes" in lib.sc_last_error()
        assert fn(fake, byref(d), sign, 2, 0, 4, fake, None, 0, None) == -1
        assert fn(fake, byref(desc(reduce=(0, 0, 1))), sign, 0, 0, 4, fake, None, 0, None) == -1
        assert fn(fake, byref(d), sign, 0, 0, 5, fake, None, 0, None) == -1 and b"unit range" in lib.sc_last_error()
        assert fn(fake, byref(many), sign, 0, 0, 640, fake, None, 0, None) == -1 and b"workspace too small" in lib.sc_last_error()


def test_request_planning():
    P = _lib
    names, mask, over, n, planes = P.jackknife_phase_request(
        ("debiased_squared_phase_lag_index", "phase_lag_index"), "trials", "trials_tapers", 5, 35)
    assert names == ["phase_lag_index", "debiased_squared_phase_lag_index"] and mask == 0x5 and over == 0 and n == 5
    assert planes == P.PLANE_SIGN_IM
    names, mask, over, n, planes = P.jackknife_phase_request("weighted_phase_lag_index", "observations", "tapers", 1, 7)
    assert names == ["weighted_phase_lag_index"] and mask == 0x2 and over == 1 and n == 7
    assert planes == P.PLANE_CSM | P.PLANE_ABS_IM
    names, mask, _, _, planes = P.jackknife_phase_request(tuple(reversed(list(P.JACKKNIFE_PHASE_MEASURES))), "trials", "trials", 9, 9)
    assert names == list(P.JACKKNIFE_PHASE_MEASURES) and mask == 0xF
    assert planes == P.PLANE_CSM | P.PLANE_ABS_IM | P.PLANE_IM_SQ | P.PLANE_SIGN_IM
    blocks, total = P.jackknife_blocks(["phase_lag_index", "debiased_squared_weighted_phase_lag_index"], 10, 3)
    assert blocks == [("phase_lag_index", 0, 90, (10, 3, 3)), ("debiased_squared_weighted_phase_lag_index", 270, 90, (10, 3, 3))]
    assert total == 540
    # the first family's helpers answer as before
    assert P.jackknife_request(("imaginary_coherence", "power"), "trials", "trials_tapers", 5, 35) == \
        (["power", "imaginary_coherence"], 0x5, 0, 5)
    assert P.jackknife_blocks(["power", "imaginary_coherence"], 10, 3) == \
        ([("power", 0, 30, (10, 3)), ("imaginary_coherence", 90, 90, (10, 3, 3))], 360)
    assert P.jackknife_split(("weighted_phase_lag_index", "power", "phase_lag_index")) == \
        (("power",), ("weighted_phase_lag_index", "phase_lag_index"))
    wpli = ("weighted_phase_lag_index",)
    for args, match in (((("wpli",), "trials", "trials_tapers", 5, 35), "unknown measure"),
                        (((), "trials", "trials_tapers", 5, 35), "empty"),
                        ((("power",), "trials", "trials_tapers", 5, 35), "unknown measure"),
                        ((wpli, "units", "trials_tapers", 5, 35), "over must be"),
                        ((wpli, "trials", "time_tapers", 5, 35), "averages over trials"),
                        ((wpli, "trials", "trials", 1, 1), "n_trials >= 2"),
                        ((wpli, "observations", "tapers", 9, 1), "n_observations >= 2"),
                        ((("debiased_squared_phase_lag_index",), "trials", "trials", 2, 2), "at least two observations"),
                        ((("debiased_squared_weighted_phase_lag_index",), "observations", "tapers", 5, 2),
                         "at least two observations")):
        with pytest.raises(ValueError, match=match):
            P.jackknife_phase_request(*args)
    # two units of one observation each are enough for PLI and wPLI; two units of two observations for the debiased ones
    assert P.jackknife_phase_request(("phase_lag_index", "weighted_phase_lag_index"), "trials", "trials", 2, 2)[3] == 2
    assert P.jackknife_phase_request(("debiased_squared_phase_lag_index",), "trials", "trials_tapers", 2, 4)[3] == 2
    with pytest.raises(ValueError, match="unknown measure 'coherence'.*'power'.*'imaginary_coherence'.*'phase_lag_index'.*"
                                         "'debiased_squared_weighted_phase_lag_index'"):
        P.jackknife_split(("coherence",))
    with pytest.raises(ValueError, match="measures is empty.*'power'.*'weighted_phase_lag_index'"):
        P.jackknife_split(())


def test_connectivity_checks_the_request_before_the_device():
    """Every ValueError of Connectivity.jackknife for the new names comes from the host: this process has no GPU."""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(1)

    def conn(shape, expectation_type):
        return sc.Connectivity(rng.standard_normal(shape) + 1j * rng.standard_normal(shape), expectation_type=expectation_type)

    with pytest.raises(ValueError, match="unknown measure 'wpli'.*'power'.*'debiased_squared_weighted_phase_lag_index'"):
        conn((2, 4, 3, 8, 3), "trials_tapers").jackknife(("power", "wpli"))
    with pytest.raises(ValueError, match="over must be"):
        conn((2, 4, 3, 8, 3), "trials_tapers").jackknife(("weighted_phase_lag_index",), over="tapers")
    with pytest.raises(ValueError, match="averages over trials"):
        conn((2, 4, 3, 8, 3), "tapers").jackknife(("power", "phase_lag_index"))
    with pytest.raises(ValueError, match="at least two observations"):
        conn((1, 2, 1, 8, 3), "trials").jackknife(("debiased_squared_weighted_phase_lag_index",))
    with pytest.raises(ValueError, match="at least two observations"):
        conn((1, 2, 1, 8, 3), "trials").jackknife(("power", "debiased_squared_phase_lag_index"))


def test_jackknife_difference():
    from spectral_connectivity_amd.statistics import JackknifeResult, jackknife_difference
    a = JackknifeResult(np.array([0.5, 0.2, np.nan]), np.array([0.6, 0.2, 0.1]), np.array([0.3, 0.1, 0.1]), "identity", 10, "trials")
    b = JackknifeResult(np.array([0.1, 0.2, 0.0]), np.array([0.1, 0.2, np.nan]), np.array([0.4, 0.1, 0.1]), "identity", 6, "trials")
    z, p = jackknife_difference(a, b)
    assert z[0] == pytest.approx(0.5 / 0.5, rel=1e-15) and z[1] == 0.0 and np.isnan(z[2])
    assert p[0] == pytest.approx(2 * scipy.stats.t.sf(1.0, 14), rel=1e-14) and p[1] == 1.0 and np.isnan(p[2])
    assert p[0] == pytest.approx(0.33428, abs=1e-5)                      # (tables: two-sided t = 1 at 14 degrees of freedom)
    zb, pb = jackknife_difference(b, a)
    assert zb[0] == -z[0] and pb[0] == p[0]
    with pytest.raises(ValueError, match="different scales"):
        jackknife_difference(a, a._replace(transform="fisher_z"))
    with pytest.raises(ValueError, match="different shapes"):
        jackknife_difference(a, JackknifeResult(np.zeros(2), np.zeros(2), np.ones(2), "identity", 6, "trials"))
