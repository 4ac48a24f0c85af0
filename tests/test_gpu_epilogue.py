"""The measures epilogue (csrc/sc_measure.hip) on records built by hand: no stage A, no stage B.  tests/epilogue_ref.py packs
chosen sums into a record -- a different number in every slot, and a fill value in every element the epilogue is documented not
to use -- and gives the nine real-valued measures in extended precision.  The one-launch kernel (measure_tile_multi_kernel: a
32 x 32 block of channel pairs per workgroup) and the one-tile kernel run at every channel count where the block geometry
changes:

  1, 2, 3 (fewer than 4), 4, 5, 12 (one tile, NB = 1: three of four waves idle), 15, 16, 17 (NB = 2: one block), 20, 31, 32,
  33 (NB = 3: the last block column holds one tile), 36, 47, 48, 49, 64, 65, 80 (NB = 5), 97, 100, 132 (vector stores into a
  partly filled tile), 260 (more than 256).

(a) against the reference: |got - ref| <= K 2^-52 cond per entry (cond: the conditioning term of epilogue_ref.measures_ref),
    NaNs at the same places.  K = 4 x the largest ratio measured on an MI355X, rounded up to a power of two
    (profiles/epilogue_accuracy.txt; a float64 NumPy evaluation of the same algebra reaches 2.4 on the CPU).
(b) bit-level identities: narrow = rounded wide, float records = double records, one-launch = one-tile, stacked = unstacked,
    parts = their host sum, exact (anti)symmetry.
(c) a NaN or 1e30 fill changes nothing.
(d) nothing is stored outside an output, aligned or not.
(e) the branch points of measure_value at their exact boundaries, a non-finite channel, one observation.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as eref                                                   # noqa: E402
from spectral_connectivity_amd import _lib, _stage_abc, engine                # noqa: E402

CHANNELS = [1, 2, 3, 4, 5, 12, 15, 16, 17, 20, 31, 32, 33, 36, 47, 48, 49, 64, 65, 80, 97, 100, 132, 260]
N_BINS, N_OBS = 3, 12
K = 16.0            # profiles/epilogue_accuracy.txt: the largest ratio on an MI355X is 3.17 (coherence magnitude); x 4, next power of two
ALL = eref.PLANES_ALL
# one launch each: (measures, planes of the record).  CSM only; unit phasors only (no CSM plane: the powers are never loaded);
# every plane; the sign plane alone
GROUPS = [
    (("coherence_magnitude", "coherence_phase", "imaginary_coherence"), eref.PLANE_CSM),
    (("phase_locking_value", "pairwise_phase_consistency"), eref.PLANE_UNIT),
    (("debiased_squared_weighted_phase_lag_index", "phase_lag_index", "pairwise_phase_consistency", "weighted_phase_lag_index"), ALL),
    (("phase_lag_index", "debiased_squared_phase_lag_index"), eref.PLANE_SIGN_IM),
]
EVERYTHING = GROUPS[2][0]
SYMMETRIC = ("coherence_magnitude", "imaginary_coherence", "phase_locking_value", "pairwise_phase_consistency",
             "debiased_squared_phase_lag_index", "debiased_squared_weighted_phase_lag_index")
ANTISYMMETRIC = ("coherence_phase", "phase_lag_index", "weighted_phase_lag_index")
OTHERS = ("power", "csm", "coherency", "plv_complex")        # the one-tile kernel's alone


def _ids(names):
    return [eref.MEASURE_IDS[n] for n in names]


def _distinct(rng, shape, signed):
    """A different float32-exact number in every slot: a permutation of 1 ... m over a power of two, in (0, 1) or (-1, 1)."""
    m = int(np.prod(shape))
    p2 = 1 << m.bit_length()
    k = rng.permutation(m).reshape(shape) + 1
    return (2.0 * k - p2) / p2 if signed else k / p2


def make_sums(C, seed):
    """Full-matrix sums from the entries i <= j (Hermitian / symmetric / antisymmetric completion; the diagonal keeps what was drawn,
    the imaginary parts too, which the epilogue must replace by 0): powers 2 ... 3 against cross terms below 1.5 in modulus,
    sum |Im s| in 1 ... 2 above sum (Im s)^2 < 1, sign sums and unit-phasor sums up to 8 of 12 observations."""
    rng = np.random.default_rng(seed)
    shape = (N_BINS, C, C)
    re, im, ur, ui, sg = (_distinct(rng, shape, True) for _ in range(5))
    ab, sq, pw = (_distinct(rng, shape, False) for _ in range(3))
    d = np.arange(C)
    full = eref.complete
    re[:, d, d] = 2.0 + pw[:, d, d]
    sums = {"s": eref.as_complex(full(re, 1), full(im, -1)), "abs_im": full(1.0 + ab, 1), "im_sq": full(sq, 1), "sign_im": full(8.0 * sg, -1),
            "unit": eref.as_complex(full(8.0 * ur, 1), full(8.0 * ui, -1))}
    for k, v in sums.items():
        assert np.array_equal(v.astype(np.complex64 if np.iscomplexobj(v) else np.float32), v), k      # float and double records: the same numbers
    return sums


@functools.lru_cache(maxsize=None)
def _case(C):
    """(sums, reference values, conditioning terms) of the channel count: computed once, shared, never written to."""
    sums = make_sums(C, 1000 + C)
    val, cond = eref.measures_ref(sums, N_OBS)
    for a in list(sums.values()) + list(val.values()) + list(cond.values()):
        a.setflags(write=False)
    return sums, val, cond


def _upload(sums, C, planes, f64, fill=0.0):
    _lib.require_gpu()
    return torch.from_numpy(eref.pack_record(sums, C, planes, np.float64 if f64 else np.float32, fill)).to("cuda:0")


@functools.lru_cache(maxsize=8)
def _record(C, planes, f64):
    return _upload(_case(C)[0], C, planes, f64)


def _multi(rec, C, planes, names, wide, n_obs=N_OBS, **kw):
    outs = engine.measure_multi(rec, C, planes, n_obs, _ids(names), wide=wide, **kw)
    assert all(o.shape == (rec.shape[-2], C, C) and o.dtype == (torch.float64 if wide else torch.float32) for o in outs)
    return {n: o.cpu().numpy() for n, o in zip(names, outs)}


def _one(rec, C, planes, name, wide, n_obs=N_OBS):
    out = engine.measure(rec, C, planes, n_obs, eref.MEASURE_IDS[name], wide=wide).cpu().numpy()
    return np.stack([out.real, out.imag], axis=-1) if np.iscomplexobj(out) else out


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _all_groups(C, f64, wide, fill=0.0, planes=None):
    """Every group through the one-launch kernel: {(group index, measure): array}."""
    sums = _case(C)[0]
    out = {}
    for g, (names, group_planes) in enumerate(GROUPS):
        p = planes or group_planes
        rec = _record(C, p, f64) if fill == 0.0 else _upload(sums, C, p, f64, fill)
        out.update({(g, n): a for n, a in _multi(rec, C, p, names, wide).items()})
    return out


# ---- (a) the reference -------------------------------------------------------------------------------------------------------------
def accuracy_table(channels=CHANNELS):
    """{measure: largest |got - ref| / (2^-52 cond)} of the one-launch kernel with wide output over float and double records of
    ``channels`` (tools/epilogue_accuracy.py prints it: profiles/epilogue_accuracy.txt)."""
    worst = {}
    for C in channels:
        _, val, cond = _case(C)
        for f64 in (False, True):
            for (g, name), got in _all_groups(C, f64, True).items():
                r = eref.worst_ratio(got, val[name], cond[name])
                worst[name] = max(worst.get(name, 0.0), r)
    return worst


@pytest.mark.parametrize("C", CHANNELS)
def test_one_launch_kernel_against_the_reference(C):
    worst = accuracy_table([C])
    print(f"\n  C = {C}: |got - ref| / (2^-52 cond): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert set(worst) == set(eref.REAL_MEASURES)
    assert max(worst.values()) <= K, worst


# ---- (b) identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CHANNELS)
def test_identities_of_the_outputs(C):
    wide = _all_groups(C, False, True)
    narrow = _all_groups(C, False, False)
    for key, w in wide.items():
        with np.errstate(over="ignore"):
            assert _same(narrow[key], w.astype(np.float32)), ("narrow output is not the rounded wide one", key)
    assert all(_same(a, wide[key]) for key, a in _all_groups(C, True, True).items()), "double records give other results than float records"
    assert all(_same(a, narrow[key]) for key, a in _all_groups(C, True, False).items())
    # a measure does not depend on its group or on the other planes of the record
    full = _all_groups(C, False, True, planes=ALL)
    assert all(_same(a, wide[key]) for key, a in full.items())
    assert _same(wide[(2, "phase_lag_index")], wide[(3, "phase_lag_index")])
    assert _same(wide[(1, "pairwise_phase_consistency")], wide[(2, "pairwise_phase_consistency")])
    by_name = {name: a for (g, name), a in wide.items()}
    off = ~np.eye(C, dtype=bool)
    for name in SYMMETRIC:
        assert _same(by_name[name], by_name[name].swapaxes(-1, -2).copy()), name
    for name in ANTISYMMETRIC:
        a = by_name[name]
        assert np.array_equal(a[:, off], -a.swapaxes(-1, -2)[:, off]) and not np.isnan(a[:, off]).any(), name
    # the one-tile kernel, measure by measure, by value with the NaNs masked
    for f64 in (False, True):
        for out_wide, multi in ((True, wide), (False, narrow)):
            rec = _record(C, ALL, f64)
            for (g, name), a in multi.items():
                one = _one(rec, C, ALL, name, out_wide)
                assert one.dtype == a.dtype and np.array_equal(np.nan_to_num(one, nan=-7.0), np.nan_to_num(a, nan=-7.0)), (name, f64, out_wide)
    # stacked: the outputs are the slices of one tensor
    rec = _record(C, ALL, False)
    for out_wide in (False, True):
        outs = engine.measure_multi(rec, C, ALL, N_OBS, _ids(EVERYTHING), wide=out_wide, stacked=True)
        assert outs[0]._base is not None and all(o._base is outs[0]._base for o in outs) and outs[0]._base.shape == (4, N_BINS, C, C)
        for name, o in zip(EVERYTHING, outs):
            assert _same(o.cpu().numpy(), (wide if out_wide else narrow)[(2, name)]), name


@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("n_parts", [2, 3])
@pytest.mark.parametrize("C", [5, 20, 33, 64, 100])
def test_parts_equal_their_host_sum(C, n_parts, f64):
    """Partial records summed by the kernel in part order = the record summed on the host in part order in the record's own type:
    four measures, and one measure alone (n_multi = 1, which only partial records reach)."""
    dtype = np.float64 if f64 else np.float32
    parts = []
    for k in range(n_parts):                             # scaled by 1/3 + k and rounded to float32: the float sums below round
        sums = make_sums(C, 7000 + 10 * C + k)
        sums = {key: (v * (1.0 / 3.0 + k)).astype(np.complex64 if np.iscomplexobj(v) else np.float32) for key, v in sums.items()}
        parts.append(eref.pack_record(sums, C, ALL, dtype))
    folded = parts[0].copy()
    for p in parts[1:]:
        folded = folded + p
    assert folded.dtype == dtype
    if not f64:
        assert (folded.astype(np.float64) != np.sum([p.astype(np.float64) for p in parts], axis=0)).any()    # (the order and the type matter)
    dev_parts = torch.from_numpy(np.stack(parts)).to("cuda:0")
    dev_folded = torch.from_numpy(folded).to("cuda:0")
    assert dev_parts.dim() == 3 and dev_parts.is_contiguous()
    for names in (EVERYTHING, ("coherence_phase",), ("phase_locking_value",), ("debiased_squared_weighted_phase_lag_index",),
                  ("coherence_magnitude", "imaginary_coherence", "debiased_squared_phase_lag_index")):
        assert _stage_abc.one_launch(_ids(names), True)
        for wide in (False, True):
            got = _multi(dev_parts, C, ALL, names, wide, n_obs=n_parts * N_OBS)
            want = _multi(dev_folded, C, ALL, names, wide, n_obs=n_parts * N_OBS)
            for name in names:
                assert np.array_equal(np.nan_to_num(got[name], nan=-7.0), np.nan_to_num(want[name], nan=-7.0)), (name, wide)
                assert np.isfinite(got[name][:, 0, C - 1]).all()


# ---- (c) poison ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("C", CHANNELS)
def test_unused_elements_are_not_read_into_a_result(C, fill):
    """The strict lower triangle of the diagonal tiles and the rows and columns >= C filled with NaN / 1e30 instead of 0: the
    one-launch kernel, the one-tile kernel (all nine, power, CSM, coherency, complex PLV) give the same bits."""
    sums = _case(C)[0]
    for f64 in (False, True):
        clean = _all_groups(C, f64, True, planes=ALL)
        poisoned = _all_groups(C, f64, True, fill=fill, planes=ALL)
        for key, a in clean.items():
            assert _same(poisoned[key], a), ("one-launch kernel", key, f64)
        rec, bad = _record(C, ALL, f64), _upload(sums, C, ALL, f64, fill)
        for name in eref.REAL_MEASURES + OTHERS:
            assert _same(_one(bad, C, ALL, name, True), _one(rec, C, ALL, name, True)), ("one-tile kernel", name, f64)


# ---- (d) stores ---------------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 64, -12345.0


def _into_guarded_buffer(rec, C, names, wide, shift):
    """The measures written into views of one sentinel-filled buffer, GUARD elements before, between and after them, the first
    view ``shift`` elements in: (outputs, everything else of the buffer)."""
    size = N_BINS * C * C
    dtype = torch.float64 if wide else torch.float32
    buf = torch.full((shift + GUARD + len(names) * (size + GUARD),), SENTINEL, dtype=dtype, device=rec.device)
    starts = [shift + GUARD + m * (size + GUARD) for m in range(len(names))]
    outs = [buf[s:s + size].view(N_BINS, C, C) for s in starts]
    assert all(o.data_ptr() == buf.data_ptr() + s * buf.element_size() for o, s in zip(outs, starts))
    ret = _stage_abc.measure_multi(engine.TorchMemory(rec.device), rec, C, ALL, N_OBS, _ids(names), wide, None, outs)
    assert all(a is b for a, b in zip(ret, outs))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    outside = np.ones(host.shape, dtype=bool)
    for s in starts:
        outside[s:s + size] = False
    return {n: host[s:s + size].reshape(N_BINS, C, C) for n, s in zip(names, starts)}, host[outside]


@pytest.mark.parametrize("C", CHANNELS)
def test_nothing_is_stored_outside_an_output(C):
    """Outputs carved out of a sentinel-filled buffer: the elements before, between and after them are untouched, the outputs
    themselves as from freshly allocated tensors."""
    for f64 in (False, True):
        rec = _record(C, ALL, f64)
        for wide in (False, True):
            want = _multi(rec, C, ALL, EVERYTHING, wide)
            got, outside = _into_guarded_buffer(rec, C, EVERYTHING, wide, 0)
            assert outside.size == 5 * GUARD and (outside == SENTINEL).all(), (f64, wide, int((outside != SENTINEL).sum()))
            assert all(_same(got[n], want[n]) for n in EVERYTHING)


@pytest.mark.parametrize("C", [20, 64, 100])
def test_misaligned_outputs_take_the_scalar_stores(C):
    """An output one element into the buffer is not 16-byte (float) / 32-byte (double) aligned: the 4-entry stores are off, the
    values and the surroundings as before."""
    rec = _record(C, ALL, False)
    for wide in (False, True):
        aligned, _ = _into_guarded_buffer(rec, C, EVERYTHING, wide, 0)
        for shift in (1, 2, 3):
            got, outside = _into_guarded_buffer(rec, C, EVERYTHING, wide, shift)
            assert (outside == SENTINEL).all(), (wide, shift)
            assert all(_same(got[n], aligned[n]) for n in EVERYTHING), (wide, shift)


# ---- (e) branch points --------------------------------------------------------------------------------------------------------------
# channels of the hand-written record: zero power; three powers around eps (pairs just below and just above eps^2); the channel that
# turns non-finite; ordinary pairs for the wPLI weight just below / just above eps and for sa^2 == sq.  C = 33: spread over the tiles
SPOTS = {5: dict(zero=1, tiny=(0, 2, 3), bad=4, w_below=(0, 4), w_above=(2, 4), wgt_zero=(3, 4)),
         33: dict(zero=1, tiny=(0, 17, 32), bad=16, w_below=(5, 20), w_above=(15, 31), wgt_zero=(18, 19))}
E = 2.0 ** -52


def branch_sums(C, bad=None, n_obs=N_OBS):
    """Integer-valued sums (so that sa^2 - sq and the comparisons are exact) with the branch points of measure_value planted:
    written into the entries i <= j, completed to full matrices at the end."""
    rng = np.random.default_rng(50 + C)
    spot = SPOTS[C]
    shape = (1, C, C)
    re, im, ur, ui = (rng.integers(-5, 6, shape).astype(np.float64) for _ in range(4))
    sa = np.abs(im) + rng.integers(2, 5, shape)
    sq = 1.0 + np.floor(rng.random(shape) * (sa * sa - 1.0))                         # 1 ... sa^2 - 1: never sa^2
    sg = rng.integers(-n_obs, n_obs + 1, shape).astype(np.float64)
    d = np.arange(C)
    re[0, d, d] = rng.integers(40, 61, C)
    ur[0, d, d] = n_obs
    planes = {"re": re, "im": im, "sa": sa, "sq": sq, "sg": sg, "ur": ur, "ui": ui}

    def put(i, j, **values):
        for key, v in values.items():
            planes[key][0, min(i, j), max(i, j)] = v

    def channel(ch, v):
        for a in planes.values():
            a[0, ch, :] = v
            a[0, :, ch] = v

    z = spot["zero"]
    channel(z, 0.0)                                       # a silent channel: zero power, zero cross terms
    # powers n eps, n eps (1 - 2^-10), n eps (1 + 2^-10): normalised products eps^2 (1 - 2^-10), eps^2 (1 + 2^-10), eps^2 (1 - 2^-20)
    a, b, c = spot["tiny"]
    for ch, f in ((a, 1.0), (b, 1.0 - 2.0 ** -10), (c, 1.0 + 2.0 ** -10)):
        for j in range(C):
            if j != ch and j != z:
                put(ch, j, re=2.0 ** -27, im=2.0 ** -26)
        re[0, ch, ch] = n_obs * E * f
    for i, j in ((a, b), (a, c), (b, c)):
        put(i, j, re=3.0 * E, im=4.0 * E)                                         # |S| / eps = 5 / 12 of the floor
    for (p, q), f in ((spot["w_below"], 1.0 - 2.0 ** -10), (spot["w_above"], 1.0 + 2.0 ** -10)):   # mean |Im s| = eps (1 -+ 2^-10)
        put(p, q, sa=n_obs * E * f, re=3.0, im=0.5 * n_obs * E, sq=0.0)
    put(*spot["wgt_zero"], sa=3.0, sq=9.0)
    if bad is not None:
        channel(spot["bad"], bad)
    full = eref.complete
    return {"s": eref.as_complex(full(re, 1), full(im, -1)), "abs_im": full(sa, 1), "im_sq": full(sq, 1), "sign_im": full(sg, -1),
            "unit": eref.as_complex(full(ur, 1), full(ui, -1))}


def _check_against_ref(sums, C, n_obs, what):
    """Both kernels, float and double records, wide output, against measures_ref: NaNs and infinities at the same places, finite
    entries within K 2^-52 cond.  Returns (the one-launch results from the double record, the reference values)."""
    val, cond = eref.measures_ref(sums, n_obs)
    kept = None
    for f64 in (False, True):
        rec = _upload(sums, C, ALL, f64)
        got = {}
        for names, _ in GROUPS:
            got.update(_multi(rec, C, ALL, names, True, n_obs=n_obs))
        for name in eref.REAL_MEASURES:
            for kernel, a in (("one-launch", got[name]), ("one-tile", _one(rec, C, ALL, name, True, n_obs=n_obs))):
                try:
                    r = eref.worst_ratio(a, val[name], cond[name])
                except AssertionError as exc:
                    raise AssertionError(f"{what}, {name}, {kernel} kernel, {'double' if f64 else 'float'} record: {exc}") from None
                assert r <= K, (what, name, kernel, f64, r)
        cy = _one(rec, C, ALL, "coherency", True, n_obs=n_obs)
        scale = np.repeat(np.hypot(*np.moveaxis(val["coherency"], -1, 0))[..., None], 2, axis=-1)
        assert eref.worst_ratio(cy, val["coherency"], scale) <= K, what
        kept = got
    return kept, val


@pytest.mark.parametrize("C", [5, 33])
def test_branch_points(C):
    spot = SPOTS[C]
    sums = branch_sums(C)
    for k, v in sums.items():
        assert np.array_equal(v.astype(np.complex64 if np.iscomplexobj(v) else np.float32), v), k
    base, val = _check_against_ref(sums, C, N_OBS, "finite record")
    # the planted entries took the branch they were planted for
    z, (a, b, c) = spot["zero"], spot["tiny"]
    others = [j for j in range(C) if j != z]
    assert (base["coherence_magnitude"][0, z, others] == 0).all() and (base["weighted_phase_lag_index"][0, z] == 0).all()
    floor = float(25.0 / 144.0)                                        # |(3 + 4i) eps / 12|^2 / eps^2
    below, above = base["coherence_magnitude"][0, a, b], base["coherence_magnitude"][0, a, c]
    assert abs(below - floor) <= K * E * floor and abs(above - floor / (1.0 + 2.0 ** -10)) <= K * E * floor
    assert abs(base["coherence_magnitude"][0, b, c] - floor) <= K * E * floor
    (i, j), (k, l) = spot["w_below"], spot["w_above"]
    assert abs(base["weighted_phase_lag_index"][0, i, j] - 0.5 * E) <= K * E * 0.5 * E                # weight -> 1
    assert abs(base["weighted_phase_lag_index"][0, k, l] - 0.5 / (1.0 + 2.0 ** -10)) <= K * E
    p, q = spot["wgt_zero"]
    dw = base["debiased_squared_weighted_phase_lag_index"]
    assert np.isnan(dw[0, p, q]) and np.isnan(dw[0, q, p]) and np.isfinite(dw[0, k, l])
    # a non-finite channel: what the reference's formulas give, and nothing changes outside its row and column
    h = spot["bad"]
    keep = np.ones((C, C), dtype=bool)
    keep[h, :] = keep[:, h] = False
    for bad in (np.inf, np.nan):
        got, _ = _check_against_ref(branch_sums(C, bad=bad), C, N_OBS, f"channel {h} = {bad}")
        for name in eref.REAL_MEASURES:
            assert np.array_equal(got[name][0][keep], base[name][0][keep], equal_nan=True), (name, bad)


@pytest.mark.parametrize("C", [5, 33])
def test_one_observation(C):
    """n = 1: PPC, debiased PLI and debiased wPLI are 0 / 0 off the diagonal, as in the reference."""
    rng = np.random.default_rng(90 + C)
    full = eref.complete
    shape = (1, C, C)
    im = full(rng.integers(1, 6, shape) * rng.choice([-1.0, 1.0], shape), -1)
    re = rng.integers(-5, 6, shape).astype(np.float64)
    phase = rng.integers(0, 4, shape)
    ur, ui = np.array([1.0, 0.0, -1.0, 0.0])[phase], np.array([0.0, 1.0, 0.0, -1.0])[phase]
    d = np.arange(C)
    re[0, d, d] = rng.integers(40, 61, C)
    ur[0, d, d], ui[0, d, d], im[0, d, d] = 1.0, 0.0, 0.0
    s, unit = eref.as_complex(full(re, 1), im), eref.as_complex(full(ur, 1), full(ui, -1))
    sums = {"s": s, "abs_im": np.abs(im), "im_sq": im * im, "sign_im": np.sign(im), "unit": unit}
    got, val = _check_against_ref(sums, C, 1, "one observation")
    off = ~np.eye(C, dtype=bool)
    for name in ("pairwise_phase_consistency", "debiased_squared_phase_lag_index", "debiased_squared_weighted_phase_lag_index"):
        assert np.isnan(val[name][0][off]).all() and np.isnan(got[name][0][off]).all(), name
    assert (np.abs(got["phase_lag_index"][0][off]) == 1).all() and (got["phase_locking_value"][0][off] == 1).all()
