"""The float32 engine at the amplitudes of real recordings: MEG in tesla (1e-13), EEG in volts (1e-6), raw 24-bit ADC counts (8e6)
and one array that mixes them -- every other GPU test feeds samples of order one.

Each channel is multiplied by a power of two, 2 ** k[c], so the scaling is exact in float32 and in float64 and commutes with every
rounding while nothing leaves the normal range.  The float64 NumPy oracle is the yardstick: PLV, PPC, PLI, both debiased measures
and power / D_c^2 are BITWISE invariant under the scaling there (asserted below: the test's own premise); coherency, coherence
magnitude, imaginary coherence and wPLI are not -- the reference's ``maximum(norm, eps)`` and ``weights < eps`` floors act at true
scale -- so for those the target is the oracle on the same scaled input.

What the float32 engine does about it ("Amplitude range of the float32 engine"): a float32 record cannot hold a sum of
(Im s)^2 of 1e-52, so stage B measures the coefficients' magnitude per channel when a request squares products ((Im s)^2) or
normalises factors (s/|s|), and accumulates a float64 record from the widened spectra when float32 would leave its normal range;
in-range data (``unit``, ``eeg``, ``adc`` here) stay on the float32 kernels, which the tests assert through the record dtype.

Records against their own route at ``unit`` (test_records_route_by_route; measured on an MI355X, see EXACT_PLANES below): the sign
sums are identical on every route at every scale; wherever the record stayed float32 (``eeg``, ``adc``; ``meg`` for the sign and unit
planes) the CSM, |Im s|, (Im s)^2 and unit planes of the one-pass and the per-plane kernels and the CSM, |Im s| and (Im s)^2 planes
of the planes-format route are bit-identical to the ``unit`` record after the exact division -- neither the rsqrt nor the
three-piece bf16 split nor the f16 pieces broke it; only the float64 fallback records (``meg``, ``ft``, ``mixed`` for (Im s)^2, ``ft``
and ``mixed`` for s/|s|) needed the 2e-6 of test_gpu_parity.test_fused_stage_b_equals_separate_kernels.  Those fallback records are
the work of ONE kernel family whatever the route asked for (sc_accumulate_f64 on the widened spectra): at ``meg``, ``ft`` and ``mixed``
the cross family's three routes, and at ``ft`` and ``mixed`` the unit family's, compare the same kernel three times -- they say
nothing about sc_fused.hip or sc_fused2.hip at those scales, which no longer see such data.  The float32 routes are covered where
the data stay float32: every route at ``unit``, ``eeg`` and ``adc``, and the unit family's (sc_nonlinear.hip's included) at ``meg``.
"""
import functools

import numpy as np
import pytest

import jackknife_ref as jref
import phase_lag_jackknife_ref as pref
import test_gpu_jackknife as tjk
import test_gpu_phase_lag_jackknife as tpjk
from conftest import device_record, unpack_record_planes
from oracle import spectral_oracle as so
from test_gpu_fp64 import close64
from test_gpu_parity import close32

pytestmark = pytest.mark.gpu
SC_PRECISIONS = ("float32", "float32+planes", "dtype")
SC_PRECISIONS_TESTS = ("test_public_measures_against_the_oracle",)      # the others drive the float32 engine explicitly

FS, NW, L, STEP, T = 200.0, 3, 64, 32, 192
GEOMETRY = dict(n_time_samples_per_window=L, n_time_samples_per_step=STEP)
MIXED = (-50, -43, -20, 0, 23)
SCALES = {"unit": (0,), "meg": (-43,), "ft": (-50,), "eeg": (-20,), "adc": (23,), "mixed": MIXED}
IN_RANGE = ("unit", "eeg", "adc")                   # the float32 selection must stay on the float32 kernels here
# one channel count per stage-B route of _stage_abc.accumulate: 6 the small one-pass VALU kernel, 40 just under the matrix-core
# crossover, 64 the matrix-core kernel with plane passes, 130 beyond 128, 5 odd (the zero pad channel)
CASES = [(6, "trials_tapers"), (40, "trials_tapers"), (64, "trials_tapers"), (130, "trials_tapers"), (5, "trials_tapers"),
         (6, "time_trials_tapers")]
INVARIANT = ("power", "phase_locking_value", "pairwise_phase_consistency", "phase_lag_index", "debiased_squared_phase_lag_index",
             "debiased_squared_weighted_phase_lag_index")
DWPLI2 = "debiased_squared_weighted_phase_lag_index"
ROUTE_TOL = 2e-6                                    # test_gpu_parity.test_fused_stage_b_equals_separate_kernels: route to route


def exponents(scale, C):
    k = SCALES[scale]
    return np.array([k[c % len(k)] for c in range(C)], dtype=np.int64)


def gains(scale, C):
    return np.ldexp(1.0, exponents(scale, C))


@functools.lru_cache(maxsize=None)
def base_series(C):
    rng = np.random.default_rng(1000 + C)
    R = 3 if C >= 130 else 5
    x = rng.standard_normal((T, R, C)) + 0.5 * rng.standard_normal((T, R, 1))
    x.setflags(write=False)
    return x


def series(C, scale):
    return base_series(C) * gains(scale, C)[None, None, :]


@functools.lru_cache(maxsize=None)
def coefficients(C, scale):
    coef, _ = so.multitaper_fft(series(C, scale), fs=FS, NW=NW, **GEOMETRY)
    coef.setflags(write=False)
    return coef


def by_bins(fn, coef, et, bin_axis, chunk=2, **kw):
    """An oracle function over the non-negative bins, two bins at a time: the oracle computes all N bins and drops the negative
    half; every quantity here is per bin, and of ``n`` bins handed in it keeps the first n // 2 + 1 -- all of one or two."""
    F = coef.shape[3] // 2 + 1
    return np.concatenate([fn(coef[..., b:min(b + chunk, F), :], et, **kw) for b in range(0, F, chunk)], axis=bin_axis)


def oracle_sums(coef, et):
    """The un-normalised sums behind the record planes, non-negative bins: {plane name: (..., F, C, C)}."""
    n = so.n_observations(coef, et)

    def total(fcn):
        with np.errstate(invalid="ignore", divide="ignore"):
            return by_bins(lambda c_, e_: so.expectation_csm_faithful(c_, e_, fcn=fcn) * n, coef, et, -3, chunk=4)
    s = total(None)
    u = total(lambda s_: s_ / np.abs(s_))
    return {"csm_re": s.real, "csm_im": total(so._zero_diag_imag), "abs_im": total(lambda s_: np.abs(so._zero_diag_imag(s_))),
            "im_sq": total(lambda s_: so._zero_diag_imag(s_) ** 2), "sign_im": total(lambda s_: np.sign(so._zero_diag_imag(s_))),
            "unit_re": u.real, "unit_im": u.imag}


_oracle_cache = {}


def oracle(C, et, scale):
    """({measure: array}, {plane: sums}) of the float64 oracle on the scaled series, computed once for the three engine selections;
    power comes divided by D_c^2.  The invariant measures are asserted bitwise equal to the oracle's at ``unit`` (and then share its
    arrays)."""
    key = (C, et, scale)
    if key in _oracle_cache:
        return _oracle_cache[key]
    coef = coefficients(C, scale)
    D = gains(scale, C)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = {name: by_bins(fn, coef, et, -2 if name == "power" else -3) for name, fn in so.MEASURES.items()}
    ref["power"] = ref["power"] / D ** 2
    sums = oracle_sums(coef, et)
    if scale != "unit":
        unit, _ = oracle(C, et, "unit")
        for name in INVARIANT:
            assert np.array_equal(ref[name], unit[name], equal_nan=True), f"the oracle's {name} is not invariant at {scale}"
            ref[name] = unit[name]
    for a in list(ref.values()) + list(sums.values()):
        a.setflags(write=False)
    _oracle_cache[key] = (ref, sums)
    return ref, sums


@pytest.fixture(scope="module")
def sc():
    import torch
    import spectral_connectivity_amd as pkg
    from spectral_connectivity_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    _lib.load()
    return pkg


def multitaper(sc, x):
    return sc.Multitaper(x, sampling_frequency=FS, time_halfbandwidth_product=NW, **GEOMETRY)


def pair_gains(D):
    return D[:, None] * D[None, :]


def device_sums(c, et, C, D, lead):
    """(sum Im s, sum |Im s|, sum (Im s)^2, record dtype) from the object's own record, each divided exactly by its pair gain."""
    from spectral_connectivity_amd import _lib
    rec = device_record(c, et, _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ)
    dev = unpack_record_planes(rec, C).reshape(lead + (4, C, C))
    g = pair_gains(D)
    planes = np.moveaxis(dev, -3, 0)
    return planes[1] / g, planes[2] / g, planes[3] / g ** 2, rec.dtype


def check_measure(name, got, ref, precision, n, ref_all, what):
    """One public measure against the oracle with the bound it has at unit amplitude (test_gpu_parity / test_gpu_fp64, f3)."""
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs from the oracle's"
    ok = ~np.isnan(ref)
    if precision == "dtype":
        if name == "coherence_phase":
            assert np.abs(np.angle(np.exp(1j * (got - ref)))[ok]).max() < 1e-8, what       # test_gpu_fp64, f3
            return
        # test_gpu_fp64, f3: the debiased ratios and PPC amplify rounding by their conditioning
        loose = name.startswith("debiased") or name == "pairwise_phase_consistency"
        close64(got, ref, rtol=1e-7 if loose else 1e-9, floor=1e-10 if loose else 1e-13, what=what)
        return
    if name in ("phase_lag_index", "debiased_squared_phase_lag_index"):
        # test_gpu_parity, f3: sign(Im s) is discontinuous -- exactness up to a handful of flipped observations
        bad = np.abs(got - ref)[ok] > 1e-6 + 1e-5 * np.abs(ref[ok])
        assert bad.mean() < 2e-3, f"{what}: {bad.sum()} of {bad.size} entries differ"
        if name == "phase_lag_index":
            assert np.abs(got - ref)[ok].max() <= 4.0 / n + 1e-6, f"{what}: more than two flipped observations in one entry"
        return
    if name == "coherence_phase":
        d = np.angle(np.exp(1j * (got - ref)))
        mag = ref_all["coherence_magnitude"]
        assert (np.abs(d[ok]) * np.sqrt(mag[ok])).max() < 2e-5, what                        # test_gpu_parity, f3
        return
    close32(got, ref, what=what)


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("C,et", CASES, ids=lambda v: str(v))
def test_public_measures_against_the_oracle(sc, C, et, scale, _engine_precision, request):
    """Every measure of so.MEASURES (power included) on the scaled series, on the three engine selections, against the oracle on
    the same series; the debiased wPLI of the float32 selections by f3's method (the three device sums against the oracle's, then
    the formula on the device sums)."""
    import torch
    precision = request.node.callspec.params["_engine_precision"]
    ref, sums = oracle(C, et, scale)
    D = gains(scale, C)
    c = sc.Connectivity.from_multitaper(multitaper(sc, series(C, scale)), expectation_type=et)
    n = c.n_observations
    iu = np.triu_indices(C, k=1)
    for name in so.MEASURES:
        got = getattr(c, name)()
        what = f"{precision} C={C} {et} {scale} {name}"
        if name == "power":
            got = got / D ** 2
        if name == DWPLI2 and precision != "dtype":
            assert np.array_equal(np.isnan(got), np.isnan(ref[name])), f"{what}: NaN pattern differs from the oracle's"
            d_im, d_abs, d_sq, _ = device_sums(c, et, C, D, ref[name].shape[:-2])
            g = pair_gains(D)
            for label, a, b in (("sum Im s", d_im, sums["csm_im"] / g), ("sum |Im s|", d_abs, sums["abs_im"] / g),
                                ("sum (Im s)^2", d_sq, sums["im_sq"] / g ** 2)):
                close32(a[..., iu[0], iu[1]], b[..., iu[0], iu[1]], what=f"{what}: {label}")
            w = d_abs ** 2 - d_sq
            with np.errstate(invalid="ignore", divide="ignore"):
                from_sums = np.where(w == 0, np.nan, (d_im ** 2 - d_sq) / w)
            up, fs_ = got[..., iu[0], iu[1]], from_sums[..., iu[0], iu[1]]
            assert np.array_equal(np.isnan(up), np.isnan(fs_)), f"{what}: NaN pattern vs the formula on the device sums"
            ok = ~np.isnan(fs_)
            assert np.abs(up[ok] - fs_[ok]).max() <= 1e-8 * max(np.abs(fs_[ok]).max(), 1.0), f"{what}: epilogue vs formula"
            assert np.array_equal(np.swapaxes(got, -1, -2)[..., iu[0], iu[1]], up, equal_nan=True), f"{what}: not symmetric"
            continue
        check_measure(name, got, ref[name], precision, n, ref, what)
    if precision != "dtype":
        # in-range data stay on the float32 kernels; out-of-range requests that square products are served in float64
        dtypes = {planes: rec[0].dtype for planes, rec in c._accum_cache.items() if isinstance(planes, int)}
        if scale in IN_RANGE:
            assert not c._device().f64, f"C={C} {scale}: the float32 selection left its spectra"
            assert all(dt == torch.float32 for dt in dtypes.values()), f"C={C} {scale}: records {dtypes}, float32 expected"
        else:
            from spectral_connectivity_amd import _lib
            sq = [dt for planes, dt in dtypes.items() if planes & _lib.PLANE_IM_SQ]
            assert sq and all(dt == torch.float64 for dt in sq), f"C={C} {scale}: the (Im s)^2 record is {sq}, float64 expected"
            if scale == "meg":
                # the verdict is per request: s / |s| is in range at tesla scale and stays on the float32 kernels, also on spectra
                # that an (Im s)^2 request has widened before
                from spectral_connectivity_amd import engine
                assert c._device()._widened is not None
                unit_record, _ = engine.accumulate(c._device(), et, _lib.PLANE_UNIT, n_freq=c._n_freq)
                assert unit_record.dtype == torch.float32, f"C={C} meg: the s/|s| record after (Im s)^2 is {unit_record.dtype}"


# ---- (b) records, route by route --------------------------------------------------------------------------------------------------
def plane_sets():
    from spectral_connectivity_amd import _lib
    return {"cross": (_lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ, ("csm_re", "csm_im", "abs_im", "im_sq")),
            "sign": (_lib.PLANE_SIGN_IM, ("sign_im",)), "unit": (_lib.PLANE_UNIT, ("unit_re", "unit_im"))}


PLANE_POWER = {"csm_re": 1, "csm_im": 1, "abs_im": 1, "im_sq": 2, "sign_im": 0, "unit_re": 0, "unit_im": 0}
ROUTES = ("one-pass", "per-plane", "planes-format")
# planes whose float32 record at scale, divided exactly, is bit for bit the same route's record at ``unit`` (measured on an MI355X);
# a float64 fallback record is held to ROUTE_TOL instead, sign sums are identical everywhere
EXACT_PLANES = {"one-pass": ("csm_re", "csm_im", "abs_im", "im_sq", "unit_re", "unit_im"),
                "per-plane": ("csm_re", "csm_im", "abs_im", "im_sq", "unit_re", "unit_im"),
                "planes-format": ("csm_re", "csm_im", "abs_im", "im_sq")}


def route_record(sc, C, et, scale, family, route, monkeypatch):
    """(planes [n_bins, n_planes, C, C] float64 divided by the pair gains, record dtype) of one route, or None where the
    planes-format kernels do not serve the family for this shape."""
    import torch
    from spectral_connectivity_amd import _stage_abc, engine
    planes, names = plane_sets()[family]
    m = multitaper(sc, series(C, scale))
    if route == "planes-format":
        monkeypatch.setenv("SC_PLANES_MIN_CHANNELS", "2")
        sp = m.device_spectra(precision="float32", planes_hint=planes)
        if sp.P is None or not _stage_abc.fused2_takes(sp.desc(et, padded=True), planes):
            return None
        accum, _ = engine.accumulate(sp, et, planes)
    else:
        sp = m.device_spectra(precision="float32")
        assert sp.P is None
        accum, _ = engine.accumulate(sp, et, planes, use_fused=route == "one-pass")
    accum = engine.fold_parts(accum)
    torch.cuda.synchronize()
    rec = unpack_record_planes(accum.cpu().numpy(), C)
    g = pair_gains(gains(scale, C))
    out = np.stack([rec[:, k] / g ** PLANE_POWER[name] for k, name in enumerate(names)], axis=1)
    return out, accum.dtype


@pytest.mark.parametrize("family", ["cross", "sign", "unit"])
@pytest.mark.parametrize("C,et", CASES, ids=lambda v: str(v))
def test_records_route_by_route(sc, C, et, family, monkeypatch):
    """The accumulator records of every stage-B route of the float32 engine at every scale: against the oracle's sums at the plain
    close32 bound, entry by entry on the upper triangle (the diagonal of the CSM too), then against the same route's record at
    ``unit``: sign sums identical, EXACT_PLANES bit for bit while the record is float32, ROUTE_TOL otherwise."""
    import torch
    _, names = plane_sets()[family]
    iu = np.triu_indices(C, k=1)
    di = np.arange(C)
    not_identical = []
    for route in ROUTES:
        unit = route_record(sc, C, et, "unit", family, route, monkeypatch)
        if unit is None:
            assert route == "planes-format"
            continue
        assert unit[1] == torch.float32, f"{route} C={C} unit: record {unit[1]}"
        for scale in SCALES:
            rec, dtype = unit if scale == "unit" else route_record(sc, C, et, scale, family, route, monkeypatch)
            if scale in IN_RANGE:
                assert dtype == torch.float32, f"{route} C={C} {scale}: record {dtype}, in-range data stay on the float32 kernels"
            _, sums = oracle(C, et, scale)
            g = pair_gains(gains(scale, C))
            for k, name in enumerate(names):
                what = f"{route} C={C} {et} {scale} {name}"
                ref = (sums[name] / g ** PLANE_POWER[name]).reshape((-1, C, C))
                got = rec[:, k]
                if name == "sign_im":
                    # (an observation within float32 rounding of Im s = 0 may flip: f3's allowance, at most two per entry)
                    diff = np.abs(got - np.rint(ref))[:, iu[0], iu[1]]      # (the oracle's mean times n: whole numbers up to rounding)
                    assert (diff > 0).mean() < 2e-3 and diff.max() <= 4.0, f"{what}: {int((diff > 0).sum())} entries, worst {diff.max()}"
                else:
                    close32(got[:, iu[0], iu[1]], ref[:, iu[0], iu[1]], what=what)
                    if name == "csm_re":
                        close32(got[:, di, di], ref[:, di, di], what=what + " (diagonal)")
                same = np.array_equal(got[:, iu[0], iu[1]], unit[0][:, k][:, iu[0], iu[1]], equal_nan=True)
                print(f"BITS {route} | C={C} {et} | {scale} | {name} | record {str(dtype).split('.')[-1]} | "
                      f"{'identical to unit' if same else 'differs from unit'}")
                if name == "sign_im" or (name in EXACT_PLANES[route] and dtype == torch.float32):
                    if not same:
                        not_identical.append(what)
                else:
                    close32(got[:, iu[0], iu[1]], unit[0][:, k][:, iu[0], iu[1]], rtol=ROUTE_TOL, atol_scale=ROUTE_TOL,
                            what=what + " vs unit")
    assert not not_identical, "not bit-identical to the same route's record at unit: " + "; ".join(not_identical)


@pytest.mark.parametrize("L", [64, 200], ids=["radix-16 kernel", "wave-per-pair kernel"])
def test_float64_transform_keeps_a_quiet_channel_beside_a_loud_one(sc, L):
    """Both fused float64 transforms pack two real channels into one complex transform: every channel of the mixed array, the one
    of 2^-50 beside the one of 2^23 included, against the oracle's coefficients of that channel alone at close64's default bound."""
    from spectral_connectivity_amd import _lib
    assert _lib.load().sc_multitaper_fft_f64_supported(L, L)
    C = 6
    D = gains("mixed", C)
    rng = np.random.default_rng(L)
    x = (rng.standard_normal((2 * L, 3, C)) + 0.5 * rng.standard_normal((2 * L, 3, 1))) * D
    kw = dict(n_time_samples_per_window=L, n_time_samples_per_step=L // 2)
    coef, _ = so.multitaper_fft(x, fs=FS, NW=NW, **kw)
    m = sc.Multitaper(x, sampling_frequency=FS, time_halfbandwidth_product=NW, **kw)
    got = np.moveaxis(m.device_spectra(precision="float64").coefficients().cpu().numpy(), 0, 3)       # (W, R, K, F, C)
    for c in range(C):
        close64(got[..., c] / D[c], coef[..., :L // 2 + 1, c] / D[c], what=f"L={L} channel {c} (2^{exponents('mixed', C)[c]})")


# ---- (c) uploaded coefficients ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["complex64", "complex128"])
@pytest.mark.parametrize("scale", ["meg", "mixed"])
def test_uploaded_coefficients(sc, scale, dtype):
    """Connectivity(coef) with the oracle's coefficients of the scaled series, as complex64 and as complex128, under the float32
    selection: PLV, PPC and the debiased wPLI against the oracle with the bounds of the measures test."""
    C, et = 6, "trials_tapers"
    ref, sums = oracle(C, et, scale)
    D = gains(scale, C)
    coef = np.ascontiguousarray(coefficients(C, scale), dtype=dtype)
    c = sc.Connectivity(coef, expectation_type=et)
    iu = np.triu_indices(C, k=1)
    for name in ("phase_locking_value", "pairwise_phase_consistency"):
        check_measure(name, getattr(c, name)(), ref[name], "float32", c.n_observations, ref, f"uploaded {dtype.__name__} {scale} {name}")
    got = c.debiased_squared_weighted_phase_lag_index()
    what = f"uploaded {dtype.__name__} {scale} {DWPLI2}"
    assert np.array_equal(np.isnan(got), np.isnan(ref[DWPLI2])), f"{what}: NaN pattern differs from the oracle's"
    d_im, d_abs, d_sq, _ = device_sums(c, et, C, D, ref[DWPLI2].shape[:-2])
    g = pair_gains(D)
    for label, a, b in (("sum Im s", d_im, sums["csm_im"] / g), ("sum |Im s|", d_abs, sums["abs_im"] / g),
                        ("sum (Im s)^2", d_sq, sums["im_sq"] / g ** 2)):
        close32(a[..., iu[0], iu[1]], b[..., iu[0], iu[1]], what=f"{what}: {label}")
    w = d_abs ** 2 - d_sq
    with np.errstate(invalid="ignore", divide="ignore"):
        from_sums = np.where(w == 0, np.nan, (d_im ** 2 - d_sq) / w)
    up, fs_ = got[..., iu[0], iu[1]], from_sums[..., iu[0], iu[1]]
    assert np.array_equal(np.isnan(up), np.isnan(fs_)), f"{what}: NaN pattern vs the formula on the device sums"
    ok = ~np.isnan(fs_)
    assert np.abs(up[ok] - fs_[ok]).max() <= 1e-8 * max(np.abs(fs_[ok]).max(), 1.0), f"{what}: epilogue vs formula"


# ---- (d) jackknife ----------------------------------------------------------------------------------------------------------------
def test_phase_lag_jackknife_at_meg(sc):
    """jackknife((PLI, wPLI), over="trials") of the float32 engine at ``meg`` against tests/phase_lag_jackknife_ref.py with the
    bounds of test_gpu_phase_lag_jackknife.py (PLI: sums of signs, exact)."""
    C, et = 6, "trials_tapers"
    coef = np.array(coefficients(C, "meg"))
    measures = ("phase_lag_index", "weighted_phase_lag_index")
    got = sc.Connectivity(coef, expectation_type=et).jackknife(measures, over="trials")
    ref = pref.jackknife(coef, et, measures, "trials")
    n = coef.shape[1]
    errors = tpjk.errors_against(got, ref, measures, "float32")
    tpjk.check(errors, "float32", "meg", n,
               bounds=lambda m, o: tpjk.F64_BOUND if m in tpjk.INTEGER else tpjk.bound("float32", o, n))


def test_power_coherence_jackknife_at_meg(sc):
    """The power / coherence / imaginary-coherence jackknife of the float32 engine at ``meg`` against tests/jackknife_ref.py with
    the bounds of test_gpu_jackknife.py."""
    C, et = 6, "trials_tapers"
    coef = np.array(coefficients(C, "meg"))
    got = tjk.device(coef, et, over="trials")
    ref = jref.jackknife(coef, et, tjk.THREE, "trials")
    n = coef.shape[1]
    errors = {(m, o): tjk.error(getattr(got[m], o), ref[m][o], o) for m in tjk.THREE for o in tjk.OUTPUTS}
    tjk.check(errors, "float32", "meg", n)
