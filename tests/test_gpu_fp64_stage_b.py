"""Stage B of the float64 engine (csrc/sc_f64.hip) at record level, every launch plan: `engine.accumulate` on uploaded complex128
coefficients against extended-precision sums of the same doubles (tests/stage_b_sums_ref.py, pinned on the CPU by
tests/test_stage_b_sums_ref.py), with bounds derived from the kernels' arithmetic -- (2 n + 18) u T for the cross-spectra,
(n + 26) u sum M for |Im s|, (n + 26) u sum M^2 for (Im s)^2, exact sign sums, (2 n + 50) u T_unit for the unit phasors; u = 2^-53,
derivations in the reference module's docstring -- on every entry of the UPPER triangle (i <= j, the diagonal included: the half
every consumer reads; the mirror half of a diagonal 16 x 16 tile is not compared) of the un-normalised records.  A dropped
observation row misses these bounds by eleven orders of magnitude.

The unit-phasor constant assumes a correctly rounded fp64 sqrt and division: the -O3 build without fast-math expands
`1.0 / sqrt(...)` of f64_load into v_rsq_f64 + the Goldschmidt / Newton correction steps of the IEEE square root and the
v_div_scale / v_rcp / v_div_fmas / v_div_fixup sequence of the IEEE division (no bare reciprocal square root).

Every test prints its worst err / bound per plane (pytest -s); profiles/f64_stage_b_bounds.txt keeps one such table as a record."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SC_PRECISION = "dtype"

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import unpack_record_planes                                   # noqa: E402
import stage_b_sums_ref as ref                                               # noqa: E402
from spectral_connectivity_amd import _lib, _stage_abc, engine              # noqa: E402

CSM, ABS, SQ, SIGN, UNIT = _lib.PLANE_CSM, _lib.PLANE_ABS_IM, _lib.PLANE_IM_SQ, _lib.PLANE_SIGN_IM, _lib.PLANE_UNIT
THREE, ALL = CSM | ABS | SQ, CSM | ABS | SQ | SIGN | UNIT
FAMILY = {CSM: "csm", ABS: "abs", SQ: "sq", SIGN: "sign", UNIT: "unit"}


def _tag(planes):
    return "+".join(name for bit, name in FAMILY.items() if planes & bit)


@functools.lru_cache(maxsize=6)
def _case(F, n_obs, C):
    """(coefficients [F, n_obs, C], their reference sums) of the data recipe, seeded by the shape; computed once per shape."""
    coef = ref.coefficients(F, n_obs, C, seed=100000 * F + 1000 * C + n_obs)
    coef.setflags(write=False)
    return coef, ref.stage_b_sums(coef)


def _upload(coef5):
    """complex128 [F, W, R, K, C] -> dense DeviceSpectra of the float64 engine."""
    _lib.require_gpu()
    F, W, R, K, C = coef5.shape
    X = torch.from_numpy(np.array(coef5, dtype=np.complex128, order="C")).to(torch.device("cuda:0"))
    sp = engine.DeviceSpectra(X, (F, W, R, K, C), (W * R * K * C, R * K * C, K * C, C), 2 * F, True, C_alloc=C)
    assert sp.f64
    return sp


def _one_run(coef):
    """[F, n_obs, C]: the observations as the trials of one window and one taper."""
    return _upload(coef[:, None, :, None, :])


def _accumulate(sp, planes, n_obs, expectation="trials_tapers"):
    """(record tensor, [n_bins, n_planes, C, C] NumPy view of it) of one engine.accumulate call."""
    accum, n = engine.accumulate(sp, expectation, planes)
    torch.cuda.synchronize()
    assert n == n_obs and accum.dtype == torch.float64 and accum.dim() == 2
    return accum, unpack_record_planes(accum.cpu().numpy(), sp.C)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _check(what, rec, planes, sums, against=None):
    """Every plane of ``rec`` inside its bound (``against``: within twice the bound of another device result); prints the ratios."""
    names = ref.record_plane_names(planes)
    worst = ref.worst_ratios(rec, names, sums, against=against, factor=1 if against is None else 2)
    print(f"  {what}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for name, r in worst.items():
        assert r <= 1.0, (what, name, r)
    return worst


@pytest.mark.parametrize("C", [5, 16, 17, 33, 47, 48, 50, 65, 81, 128, 129, 200, 256])
def test_every_launch_plan(C, debug_env):
    """Two bins of 70 observations (nine 8-row chunks of the CSM kernel, five 16-row chunks of the plane kernels, the last partial
    in both); signals: MAX_SLOTS 1 (5, 16), 3 (17, 33, 47, 48), 5 (50, 65, 81) and 9 (128 ... 256), one to four tile groups with
    the last partial (129: 45 tiles, 200: 91, 256: 136), CP = 32 NB32 wider than 16 NB (5, 17, 33, 65, 81, 129, 200), the last
    count of nonlinear_f64_kernel (47) and the first of the block kernel (48), one to four 64-blocks with trailing blocks of 1
    (65, 129), 8 (200) and 64 channels; every bin in 1, 2, 3, 7 and 16 parts (SC_F64_SPLIT; 7 and 16 leave parts without a chunk).
    Requests: CSM + |Im s| + (Im s)^2 in one call (from 48 signals the planes on the forked side stream), sign alone, unit alone.
    Every plane inside its bound, every split within twice the bound of split 1, every call equal to its repeat bit for bit."""
    F, n_obs = 2, 70
    coef, sums = _case(F, n_obs, C)
    assert sums["near_zero"] == 0
    sp = _one_run(coef)
    print(f"\n {C} signals, err / bound per (parts, request):")
    whole = {}
    for split in (1, 2, 3, 7, 16):
        debug_env("SC_F64_SPLIT", split)
        for planes in (THREE, SIGN, UNIT):
            a, rec = _accumulate(sp, planes, n_obs)
            b, _ = _accumulate(sp, planes, n_obs)
            assert _same_bits(a, b), (split, _tag(planes), "two calls differ")
            _check(f"{C:3d} signals, {split:2d} parts, {_tag(planes):10s}", rec, planes, sums)
            if split == 1:
                whole[planes] = rec
            else:
                w = ref.worst_ratios(rec, ref.record_plane_names(planes), sums, against=whole[planes], factor=2)
                assert max(w.values()) <= 1.0, (split, _tag(planes), "differs from the unsplit record", w)


@pytest.mark.parametrize("n_obs", [1, 7, 8, 9, 15, 16, 17, 31, 33, 255, 257, 520, 1031])
@pytest.mark.parametrize("C", [40, 96])
def test_depth(C, n_obs, debug_env):
    """One bin of 1 ... 1031 observations around the chunk sizes (8 and 16 rows), 40 signals (nonlinear_f64_kernel) and 96 (the
    block kernel, a 32-channel trailing block), all five families in one call; the split left to the engine (f64_pick_split: two
    parts at 520 observations, four at 1031, one below 497) and forced to 2 and 3.  One observation: the sign sums are exactly
    +-1 off the diagonal and 0 on it, PLI likewise, and every unit-phasor sum has modulus 1 to the bound of its two parts."""
    coef, sums = _case(1, n_obs, C)
    assert sums["near_zero"] == 0
    sp = _one_run(coef)
    print(f"\n {C} signals x {n_obs} observations, err / bound per forced split:")
    for split in (None, 2, 3):
        debug_env("SC_F64_SPLIT", split)
        a, rec = _accumulate(sp, ALL, n_obs)
        _check(f"{C:3d} signals x {n_obs:4d}, split {split}", rec, ALL, sums)
        if n_obs == 1:
            strict = np.triu(np.ones((C, C), dtype=bool), 1)
            g = rec[0, 4]
            assert np.all(np.abs(g[strict]) == 1.0) and np.all(np.diag(g) == 0.0)
            pli = engine.measure(a, C, ALL, 1, _lib.M_PLI).cpu().numpy().reshape(C, C)
            assert np.all(np.abs(pli[~np.eye(C, dtype=bool)]) == 1.0) and np.all(np.diag(pli) == 0.0)
            assert np.array_equal(pli[strict], g[strict]) and np.array_equal(pli.T[strict], -g[strict])
            b = ref.bounds(sums)
            upper = np.triu(np.ones((C, C), dtype=bool))
            off = np.abs(np.hypot(rec[0, 5], rec[0, 6]) - 1.0)[upper]
            assert np.all(off <= (b["U_re"][0] + b["U_im"][0])[upper].astype(np.float64))


@pytest.mark.parametrize("C", [50, 129, 256])
def test_no_block_switch(C, debug_env):
    """SC_F64_NO_BLOCK=1: nonlinear_f64_kernel beyond its 47 signals -- 3, 15 and 36 blocks of 32 x 32, sets of 2 (|Im s| and
    (Im s)^2 together) and 3 (sign) -- inside the same bounds; the CSM and unit planes, which the switch does not reach, bit for bit
    as without it.  Whole bins and bins in two parts (the kernel itself never splits)."""
    F, n_obs = 2, 70
    coef, sums = _case(F, n_obs, C)
    sp = _one_run(coef)
    print(f"\n {C} signals, SC_F64_NO_BLOCK, err / bound:")
    for split in (None, 2):
        debug_env("SC_F64_SPLIT", split)
        debug_env("SC_F64_NO_BLOCK", None)
        default = {planes: _accumulate(sp, planes, n_obs)[0] for planes in (THREE, SIGN, UNIT)}
        debug_env("SC_F64_NO_BLOCK", 1)
        for planes in (THREE, SIGN, UNIT):
            a, rec = _accumulate(sp, planes, n_obs)
            _check(f"{C:3d} signals, split {split}, {_tag(planes):10s}", rec, planes, sums)
            if planes == UNIT:
                assert _same_bits(a, default[planes])
            if planes == THREE:
                per_plane = a.shape[1] // 4
                assert _same_bits(a[:, :2 * per_plane], default[planes][:, :2 * per_plane])


def test_no_fork_switch(debug_env):
    """SC_F64_NO_FORK=1 at 65 signals: the plane kernels behind the CSM kernel on the caller's stream instead of the side
    stream -- the same kernels, so the same record bit for bit."""
    F, n_obs, C = 2, 70, 65
    coef, sums = _case(F, n_obs, C)
    sp = _one_run(coef)
    print(f"\n {C} signals, SC_F64_NO_FORK, err / bound:")
    for split in (None, 3):
        debug_env("SC_F64_SPLIT", split)
        debug_env("SC_F64_NO_FORK", None)
        default, _ = _accumulate(sp, ALL, n_obs)
        debug_env("SC_F64_NO_FORK", 1)
        a, rec = _accumulate(sp, ALL, n_obs)
        _check(f"{C:3d} signals, split {split}", rec, ALL, sums)
        assert _same_bits(a, default)


@pytest.mark.parametrize("C", [33, 129, 256])
def test_sixteen_row_chunks_of_the_csm_kernel(C, debug_env):
    """SC_F64_OC=16 (a diagnostic form of csm_f64_kernel: 16 observation rows per staged chunk instead of 8), CSM and unit planes:
    inside the same bounds; the |Im s|, (Im s)^2 and sign planes, which it does not reach, bit for bit as without it."""
    F, n_obs = 2, 70
    coef, sums = _case(F, n_obs, C)
    sp = _one_run(coef)
    print(f"\n {C} signals, SC_F64_OC=16, err / bound:")
    for split in (None, 3):
        debug_env("SC_F64_SPLIT", split)
        debug_env("SC_F64_OC", None)
        default, _ = _accumulate(sp, ALL, n_obs)
        debug_env("SC_F64_OC", 16)
        a, rec = _accumulate(sp, ALL, n_obs)
        _check(f"{C:3d} signals, split {split}", rec, ALL, sums)
        per_plane = a.shape[1] // 7
        assert _same_bits(a[:, 2 * per_plane:5 * per_plane], default[:, 2 * per_plane:5 * per_plane])


@pytest.mark.parametrize("C", [20, 50])
@pytest.mark.parametrize("expectation", list(_lib.EXPECTATION_AXES))
def test_reduced_axes_that_are_not_one_linear_run(expectation, C, debug_env):
    """Spectra [2 bins][3 windows][2 trials][5 tapers], all seven expectation types: 1 ... 15 groups of 2 ... 30 observations,
    linear runs (obs_stride > 0) and the ones that are not (windows and tapers with the trials kept: obs_stride == 0, every row
    through sc_obs_offset) in all three kernels, against the sums of the correspondingly grouped observations."""
    F, W, R, K = 2, 3, 2, 5
    coef, _ = _case(F, W * R * K, C)
    coef5 = coef.reshape(F, W, R, K, C)
    grouped, n_obs = ref.grouped_observations(coef5, _lib.EXPECTATION_AXES[expectation])
    sums = ref.stage_b_sums(grouped)
    assert sums["near_zero"] == 0
    sp = _upload(coef5)
    print(f"\n {C} signals, {expectation}: {grouped.shape[0] // F} groups x {n_obs} observations, err / bound:")
    for split in (None, 2):
        debug_env("SC_F64_SPLIT", split)
        _, rec = _accumulate(sp, ALL, n_obs, expectation)
        assert rec.shape[0] == grouped.shape[0]
        _check(f"{C:3d} signals, {expectation}, split {split}", rec, ALL, sums)


def test_which_fills_one_family_and_leaves_the_others(debug_env):
    """A record of all five families brought by the caller (`out`), pre-filled with a sentinel and filled one family per call
    (`which`): after each call only that family's planes have changed, none of them holds the sentinel any more, and the end
    state is the record of one call for all five, bit for bit.  65 signals, every bin in three parts: the scratch records and
    the combine kernel must keep to the planes of the family."""
    F, n_obs, C = 2, 70, 65
    coef, sums = _case(F, n_obs, C)
    sp = _one_run(coef)
    debug_env("SC_F64_SPLIT", 3)
    one_call, _ = _accumulate(sp, ALL, n_obs)
    mem = engine.TorchMemory(sp.device)
    sentinel = -7.25e250
    rec = torch.full_like(one_call, sentinel)
    slots = engine.plane_slots(ALL)
    per_plane = rec.shape[1] // 7
    for bit in (UNIT, ABS, CSM, SIGN, SQ):
        before = rec.clone()
        out, n = _stage_abc.accumulate(mem, sp, "trials_tapers", ALL, None, bit, rec)
        torch.cuda.synchronize()
        assert out is rec and n == n_obs
        first, width = slots[bit]
        mine = slice(first * per_plane, (first + width) * per_plane)
        assert not bool((rec[:, mine] == sentinel).any()), FAMILY[bit]
        assert _same_bits(rec[:, :mine.start], before[:, :mine.start]), FAMILY[bit]
        assert _same_bits(rec[:, mine.stop:], before[:, mine.stop:]), FAMILY[bit]
    assert _same_bits(rec, one_call)
    print()
    _check(f"{C} signals, one family per call", unpack_record_planes(rec.cpu().numpy(), C), ALL, sums)


def test_zero_channels(debug_env):
    """65 signals with channel 64 (the one-channel trailing block) and channel 3 identically zero: the unit-phasor planes are NaN
    in exactly their rows and columns (0 / 0, like the reference's s / |s|) and finite elsewhere -- the zero-filled rows past the
    70th observation of the last chunk leak none -- and every other plane is exactly 0 there."""
    F, n_obs, C = 2, 70, 65
    coef = np.array(_case(F, n_obs, C)[0])
    zero = [3, 64]
    coef[:, :, zero] = 0
    sums = ref.stage_b_sums(coef)
    assert sums["near_zero"] == F * n_obs * (2 * (C - 1) - 1)              # the pairs with a zero channel (d = 0 exactly), no other
    sp = _one_run(coef)
    dead = np.zeros((C, C), dtype=bool)
    dead[zero, :] = dead[:, zero] = True
    upper = np.triu(np.ones((C, C), dtype=bool))
    print()
    for split in (None, 3):
        debug_env("SC_F64_SPLIT", split)
        _, rec = _accumulate(sp, ALL, n_obs)
        _check(f"{C} signals, two of them zero, split {split}", rec, ALL, sums)
        for k in (5, 6):
            assert np.all(np.isnan(rec[:, k][:, dead & upper])) and np.all(np.isfinite(rec[:, k][:, ~dead & upper]))
        for k in range(5):
            assert np.all(rec[:, k][:, dead & upper] == 0.0) and np.all(np.isfinite(rec[:, k][:, upper]))


def test_more_than_256_signals():
    """270 signals through engine._accumulate_blocked (blocks of 128, 128 and 14 channels: three requests of 256 and 142 signals
    whose tiles are copied into the full record), all five families: the same bounds on the assembled record."""
    F, n_obs, C = 1, 70, 270
    coef, sums = _case(F, n_obs, C)
    assert sums["near_zero"] == 0
    sp = _one_run(coef)
    accum, n = engine._accumulate_blocked(sp, "trials_tapers", ALL, None, None, 1)
    torch.cuda.synchronize()
    assert n == n_obs and accum.dtype == torch.float64
    print()
    _check(f"{C} signals, tiled", unpack_record_planes(accum.cpu().numpy(), C), ALL, sums)
