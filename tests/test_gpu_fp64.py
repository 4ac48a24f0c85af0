"""The float64 engine -- what `Connectivity(dtype=numpy.complex128)`, the reference's default dtype, runs: float64
transform, complex128 spectra, cross-spectra on the fp64 matrix cores, double records, float64 measures -- against the
golden vectors of the real reference and the NumPy oracle, ELEMENTWISE and RELATIVE, no absolute floor beyond 1e-13 of
the array maximum (the reference's own rounding).  The float32 engine's tests (test_gpu_parity.py ...) state the f32
bounds; here the bar is the reference's arithmetic itself.  Stage B of this engine at record level -- every launch plan of
csrc/sc_f64.hip, split bins, the SC_F64_* switches, against extended-precision sums with derived bounds -- is in
tests/test_gpu_fp64_stage_b.py."""
import numpy as np
import pytest

from oracle import spectral_oracle as so
from fp64_device_ref import measures_fp64, relative_error_report, spectra_fp64, sums_fp64

pytestmark = pytest.mark.gpu
SC_PRECISION = "dtype"          # conftest: leave the package default (dtype decides the engine)
FS = 1000.0


def close64(a, b, rtol=1e-9, floor=1e-13, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(b)
    if not ok.any():
        return
    scale = np.abs(b[ok]).max()
    err = np.abs(a[ok] - b[ok])
    worst = (err / (rtol * np.abs(b[ok]) + floor * scale + 1e-300)).max()
    if what.startswith("!"):
        print(f"  {what}: max err {err.max():.3e} (scale {scale:.3e}), worst err/bound {worst:.2f}")
    assert worst <= 1.0, f"{what}: max err {err.max():.3e} (scale {scale:.3e}), worst err/bound {worst:.2f}"


@pytest.fixture(scope="module")
def sc():
    import spectral_connectivity_amd as pkg
    return pkg


def test_dtype_selects_the_engine(sc):
    import torch
    x = np.random.default_rng(0).standard_normal((128, 3, 4))
    m = sc.Multitaper(x, sampling_frequency=100.0, time_halfbandwidth_product=2)
    c128 = sc.Connectivity.from_multitaper(m)                                # the reference's default dtype
    c64 = sc.Connectivity.from_multitaper(m, dtype=np.complex64)
    assert c128._device().X.dtype == torch.complex128 and c64._device().X.dtype == torch.complex64
    a, b = c128.coherence_magnitude(), c64.coherence_magnitude()
    assert a.dtype == b.dtype == np.float64
    off = ~np.eye(4, dtype=bool)
    assert 0 < np.abs(a - b)[..., off].max() < 1e-5                          # two engines, same quantity
    coef, _ = so.multitaper_fft(x, fs=100.0, NW=2)
    close64(m.fft(), coef, what="Multitaper.fft() is float64 like the reference's")
    with pytest.raises(ValueError, match="complex64 or numpy.complex128"):
        sc.Connectivity.from_multitaper(m, dtype=np.float32)
    zc, _ = so.multitaper_fft(x + 1j * x[::-1], fs=100.0, NW=2)                # complex series: two-sided, like the reference's
    close64(sc.Multitaper(x + 1j * x[::-1], sampling_frequency=100.0, time_halfbandwidth_product=2).fft(), zc, what="complex series")


def test_f1_f2_transform_and_measures(sc, golden):
    g = golden("f1_cfg1")
    m = sc.Multitaper(g["x"], sampling_frequency=float(g["fs"]), time_halfbandwidth_product=float(g["NW"]))
    close64(m.fft(), g["fft"], what="fft")
    c = sc.Connectivity.from_multitaper(m)
    close64(c.power(), g["power"], what="power")
    close64(c.coherency(), g["coherency"], what="coherency")
    close64(c.coherence_magnitude(), g["coherence_magnitude"], what="coherence")
    g = golden("f2_detrend")
    for det in ("constant", "linear", None):
        m = sc.Multitaper(g["x"], sampling_frequency=float(g["fs"]), time_halfbandwidth_product=float(g["NW"]),
                          detrend_type=det)
        close64(m.fft(), g[f"fft_{det}"], what=f"fft detrend={det}")


@pytest.mark.parametrize("et", list(so.EXPECTATION_AXES))
def test_f3_every_measure_every_expectation(sc, golden, et):
    g = golden("f3_windows_all_measures")
    m = sc.Multitaper(g["x"], sampling_frequency=float(g["fs"]), time_halfbandwidth_product=float(g["NW"]),
                      n_time_samples_per_window=int(g["L"]), n_time_samples_per_step=int(g["step"]))
    c = sc.Connectivity.from_multitaper(m, expectation_type=et)
    for name in so.MEASURES:
        ref, got = g[f"{et}__{name}"], getattr(c, name)()
        if name == "coherence_phase":
            ok = ~np.isnan(ref)
            assert np.abs(np.angle(np.exp(1j * (got - ref)))[ok]).max() < 1e-8, f"{et}/phase"
            continue
        # the debiased ratios over as few as three observations amplify rounding by their conditioning
        loose = name.startswith("debiased") or name in ("pairwise_phase_consistency",)
        close64(got, ref, rtol=1e-7 if loose else 1e-9, floor=1e-10 if loose else 1e-13, what=f"{et}/{name}")


@pytest.mark.parametrize("tag,kw", [
    ("L250", dict(n_time_samples_per_window=250)),
    ("L250_N300", dict(n_time_samples_per_window=250, n_fft_samples=300)),
    ("L255", dict(n_time_samples_per_window=255)),
    ("L256_N255", dict(n_time_samples_per_window=256, n_fft_samples=255)),
    ("dur_step", dict(time_window_duration=0.8, time_window_step=0.29)),
])
def test_f4_lengths(sc, golden, tag, kw):
    g = golden("f4_lengths")
    m = sc.Multitaper(g["x"], sampling_frequency=float(g["fs"]), time_halfbandwidth_product=float(g["NW"]), **kw)
    close64(m.fft(), g[f"{tag}__fft"], what=f"{tag} fft")
    c = sc.Connectivity.from_multitaper(m)
    close64(c.coherence_magnitude(), g[f"{tag}__coherence_magnitude"], what=f"{tag} coherence")
    close64(c.power(), g[f"{tag}__power"], what=f"{tag} power")


def test_f7_edges_and_uploaded_coefficients(sc, golden):
    g = golden("f7_edges")
    m = sc.Multitaper(g["zero__x"], sampling_frequency=100.0, time_halfbandwidth_product=2)
    c = sc.Connectivity.from_multitaper(m)
    for name in ("coherence_magnitude", "imaginary_coherence", "weighted_phase_lag_index"):
        close64(getattr(c, name)(), g[f"zero__{name}"], what=f"zero-power {name}")
    coef, _ = so.multitaper_fft(g["zero__x"], fs=100.0, NW=2)
    c = sc.Connectivity(coef)                                                # raw complex128 upload, all N bins
    close64(c.coherence_magnitude(), so.coherence_magnitude(coef), what="uploaded coherence")
    close64(c.weighted_phase_lag_index(), so.weighted_phase_lag_index(coef), what="uploaded wpli")


@pytest.mark.parametrize("C,R,et", [(32, 20, "trials_tapers"), (128, 6, "trials_tapers"), (40, 5, "trials"),
                                    (19, 7, "time_trials_tapers"), (160, 3, "trials_tapers"), (255, 2, "tapers")])
def test_seeded_vs_oracle_multi_tile(sc, C, R, et):
    """1 ... 16 channel blocks, odd sizes, every tile-group / block-set instantiation of the fp64 kernels."""
    rng = np.random.default_rng(100 + C)
    T = 384
    x = rng.standard_normal((T, R, C))
    t = np.arange(T) / 500.0
    x += 0.6 * np.sin(2 * np.pi * 45 * t)[:, None, None] * rng.standard_normal(C)[None, None, :]
    kw = dict(n_time_samples_per_window=128, n_time_samples_per_step=64)
    m = sc.Multitaper(x, sampling_frequency=500.0, time_halfbandwidth_product=2, **kw)
    c = sc.Connectivity.from_multitaper(m, expectation_type=et)
    coef, _ = so.multitaper_fft(x, fs=500.0, NW=2, **kw)
    csm = so.expectation_csm_gemm(coef, et)
    close64(c.coherency(), so.coherency(coef, et, csm=csm), what="coherency")
    close64(c.imaginary_coherence(), so.imaginary_coherence(coef, et, csm=csm), what="imag coh")
    close64(c.power(), so.power(coef, et), what="power")
    if C <= 40:
        close64(c.weighted_phase_lag_index(), so.weighted_phase_lag_index(coef, et), what="wpli")
        close64(c.phase_locking_value(), so.phase_locking_value(coef, et), what="plv")
        close64(c.phase_lag_index(), so.phase_lag_index(coef, et), what="pli")
        close64(c.debiased_squared_weighted_phase_lag_index(),
                so.debiased_squared_weighted_phase_lag_index(coef, et), rtol=1e-7, floor=1e-10, what="dwpli2")


def test_granger_canonical_mvar_global_from_double_records(sc, golden):
    g = golden("f5_granger")
    for tag, kw in (("ding2", dict(time_halfbandwidth_product=1)),
                    ("bacc3", dict(time_halfbandwidth_product=2, n_time_samples_per_window=250))):
        c = sc.Connectivity.from_multitaper(sc.Multitaper(g[f"{tag}__x"], sampling_frequency=200.0, **kw))
        got, ref = c.pairwise_spectral_granger_prediction(), g[f"{tag}__granger"]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
        both = ~np.isnan(ref)
        # Wilson stops at max |dG| < 1e-8: the factor, hence the log-ratio, is defined to ~1e-8
        assert np.max(np.abs(got[both] - ref[both])) <= 2e-7 * np.nanmax(ref), tag
    g = golden("f6_canonical")
    m = sc.Multitaper(g["x"], sampling_frequency=float(g["fs"]), time_halfbandwidth_product=float(g["NW"]),
                      n_time_samples_per_window=int(g["L"]))
    cc, labels = sc.Connectivity.from_multitaper(m).canonical_coherence(g["group_labels"])
    close64(cc, g["canonical_coherence"], rtol=1e-7, floor=1e-8, what="canonical coherence")   # Jacobi sweeps stop at 1e-9
    g = golden("f9_mvar")
    m = sc.Multitaper(g["var3__x"], sampling_frequency=128.0, time_halfbandwidth_product=2, n_time_samples_per_window=256)
    c = sc.Connectivity.from_multitaper(m)
    close64(c._minimum_phase_factor, g["var3__minimum_phase_factor"], rtol=1e-6, floor=1e-7, what="minimum phase factor")
    for name in ("directed_transfer_function", "partial_directed_coherence"):
        close64(getattr(c, name)(), g[f"var3__{name}"], rtol=1e-6, floor=1e-6, what=name)
    g = golden("f10_global")
    m = sc.Multitaper(g["x"], sampling_frequency=256.0, time_halfbandwidth_product=2, n_time_samples_per_window=128)
    vals, _ = sc.Connectivity.from_multitaper(m).global_coherence(max_rank=2)
    close64(vals, g["rank2__values"], rtol=1e-8, floor=1e-10, what="global coherence")


def synth(T, R, C, tone, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, R, C)).astype(np.float32)
    t = np.arange(T) / FS
    x += (0.5 * np.sin(2 * np.pi * tone * t[:, None, None] + 2 * np.pi * np.arange(C)[None, None, :] / C)).astype(np.float32)
    return x


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3", "cfg5"])
def test_full_depth_elementwise_relative(sc, cfg):
    """The BASELINE configurations at FULL size through the float64 engine against the float64 torch restatement of
    the oracle (tests/fp64_device_ref.py, pinned to the NumPy oracle in tests/test_gpu_full_depth.py): 1e-5 relative
    on EVERY entry -- the bar north_star states, with no floor beyond 1e-13 of the maximum; the achieved error is
    ~1e-12 and printed."""
    if cfg == "cfg2":
        x, NW, kw, names = synth(1024, 100, 32, 40.0, 2), 3, {}, ["power", "coherency", "weighted_phase_lag_index"]
    elif cfg == "cfg3":
        x, NW, kw = synth(1024, 1000, 128, 60.0, 3), 4, dict(n_time_samples_per_window=256, n_time_samples_per_step=128)
        names = ["power", "coherency", "coherence_magnitude", "weighted_phase_lag_index"]
    else:
        rng = np.random.default_rng(5)
        x = rng.standard_normal((1024, 500, 256)).astype(np.float32)
        x += (0.6 * np.repeat(rng.standard_normal((1024, 500, 16)), 16, axis=2)).astype(np.float32)
        NW, kw, names = 3, {}, ["power", "coherency"]
    m = sc.Multitaper(x, sampling_frequency=FS, time_halfbandwidth_product=NW, **kw)
    c = sc.Connectivity.from_multitaper(m)
    X = spectra_fp64(x, m.tapers, FS, m.n_time_samples_per_window, m.n_time_samples_per_step, m.n_fft_samples)
    csm, ab = sums_fp64(X, want_abs="weighted_phase_lag_index" in names)
    n_obs = X.shape[2] * X.shape[3]
    del X
    ref = measures_fp64(csm, ab, n_obs)
    print(f"\n{cfg}, float64 engine:")
    for name in names:
        got = getattr(c, name)()
        mx, q999, frac = relative_error_report(got, ref[name], floor=1e-9)
        print(f"  {name}: max rel err {mx:.2e} (99.9th pct {q999:.2e}) over {100 * frac:.2f} % of the entries")
        close64(got, ref[name], rtol=1e-5, floor=1e-13, what=f"{cfg} {name}")
        assert mx < 1e-7, f"{cfg} {name}: {mx}"
    if cfg == "cfg5":
        # canonical coherence of the 16 groups x 513 bins at full depth: sigma_max(L_g^-1 S_gh L_h^-H)^2 from the float64
        # reference spectra in NumPy (equal to the reference's SVD form when n_obs >= group size: pinned against the oracle
        # at 24 trials in tests/test_gpu_configs.py), element by element
        labels = np.repeat(np.arange(16), 16)
        S = (csm / n_obs).cpu().numpy()[0]                                   # (F, C, C)
        Linv = []
        for g in range(16):
            sl = slice(16 * g, 16 * g + 16)
            Linv.append(np.linalg.inv(np.linalg.cholesky(S[:, sl, sl])))
        ref_cc = np.full((S.shape[0], 16, 16), np.nan)
        for g in range(16):
            for h in range(g + 1, 16):
                M = Linv[g] @ S[:, 16 * g:16 * g + 16, 16 * h:16 * h + 16] @ np.conj(np.swapaxes(Linv[h], -1, -2))
                ref_cc[:, g, h] = ref_cc[:, h, g] = np.linalg.svd(M, compute_uv=False)[:, 0] ** 2
        cc, lab = c.canonical_coherence(labels)
        assert np.array_equal(lab, np.arange(16)) and cc.shape == (1,) + ref_cc.shape
        mx, q999, frac = relative_error_report(cc[0], ref_cc, floor=1e-9)
        print(f"  canonical_coherence: max rel err {mx:.2e} (99.9th pct {q999:.2e}) over {100 * frac:.2f} % of the entries")
        close64(cc[0], ref_cc, rtol=1e-6, floor=1e-13, what="cfg5 canonical coherence")


def test_f11_band_statistics_float64(sc, golden):
    """phase_slope_index / group_delay / delay on the float64 engine's coherency: equal to the reference's outputs."""
    g = golden("f11_post")
    c = sc.Connectivity.from_multitaper(sc.Multitaper(g["x"], sampling_frequency=500.0, time_halfbandwidth_product=3))
    close64(c.coherency(), g["coherency"], what="f11 coherency")
    res = float(g["frequency_resolution"])
    close64(c.phase_slope_index(), g["psi_all"], rtol=1e-8, floor=1e-10, what="psi")
    close64(c.phase_slope_index([10, 200], res), g["psi_band_res"], rtol=1e-8, floor=1e-10, what="psi band")
    d, s_, r = c.group_delay([10, 200], res)
    for a, key in ((d, "group_delay"), (s_, "group_slope"), (r, "group_r")):
        np.testing.assert_allclose(a, g[key], rtol=1e-12, atol=0, equal_nan=True, err_msg=key)
    np.testing.assert_allclose(c.delay([10, 200], n_range=2), g["delay_band"], rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.parametrize("N,L,C,det", [(256, 256, 128, "constant"), (64, 50, 5, "linear"), (128, 128, 33, None),
                                       (512, 400, 18, "constant"), (1024, 1024, 7, "linear"), (200, 200, 70, "linear"),
                                       (250, 250, 3, "constant"), (400, 300, 9, None), (500, 500, 16, "constant"),
                                       (1000, 1000, 6, "linear"), (256, 256, 1, "constant")])
def test_fused_float64_transform_matches_oracle_and_rocfft(sc, N, L, C, det):
    """Stage A of the float64 engine as one kernel (sc_mtfft_f64.hip) against the float64 oracle -- 1e-12 of the spectrum's
    scale -- and against the three-pass route it replaces (still the path of every other length)."""
    import torch
    from oracle import spectral_oracle as so
    from spectral_connectivity_amd import _lib, engine
    assert _lib.load().sc_multitaper_fft_f64_supported(L, N) == 1
    assert _lib.load().sc_multitaper_fft_f64_supported(300, 300) == 0
    rng = np.random.default_rng(N + C)
    R, step = 3, max(L // 2, 1)
    T = L + 2 * step
    x = rng.standard_normal((T, R, C)) + 5.0 + np.linspace(0, 2, T)[:, None, None]
    if C >= 4:
        x[:, :, 2] = 0.0                                      # a silent channel: exact zeros
    kw = dict(n_time_samples_per_window=L, n_time_samples_per_step=step, n_fft_samples=N)
    coef, _ = so.multitaper_fft(x, fs=200.0, NW=2.5, detrend_type=det, **kw)
    m = sc.Multitaper(x, sampling_frequency=200.0, time_halfbandwidth_product=2.5, detrend_type=det, **kw)
    xd = torch.from_numpy(x).cuda()
    h = torch.from_numpy(np.ascontiguousarray(m.tapers.T / 200.0)).cuda()
    W = m.n_time_windows
    ref = coef[..., : N // 2 + 1, :]
    scale = np.abs(ref).max()
    got = {}
    for fused in (True, False):
        sp = engine.multitaper_spectra_f64(xd, h, L, step, N, W, det, use_fused=fused)
        got[fused] = np.moveaxis(sp.coefficients().cpu().numpy(), 0, 3)
        assert got[fused].shape == ref.shape
        assert np.abs(got[fused] - ref).max() <= 1e-12 * scale, (fused, np.abs(got[fused] - ref).max() / scale)
    if C >= 4 and det != "linear":
        assert np.all(got[True][..., 2] == 0)
    assert np.all(got[True][..., 0, :].imag == 0)            # DC exactly real
    if N % 2 == 0:
        assert np.all(got[True][..., N // 2, :].imag == 0)   # Nyquist exactly real
    close64(m.fft(), coef, rtol=1e-9, floor=1e-12, what="Multitaper.fft()")


def test_cfg4_full_size_granger_elementwise(sc):
    """BASELINE configs[3] at full size (64 ch x 200 trials x 4096 samples): pairwise spectral Granger prediction of the
    float64 engine against the oracle, element by element.  A pair's prediction depends on its two channels only, so the
    CPU oracle is handed just the channels of the pairs checked (the full coefficient array would be 34 GB)."""
    from oracle import spectral_oracle as so
    rng = np.random.default_rng(4)
    C, T, R = 64, 4096, 200
    e = rng.standard_normal((T + 200, R, C))
    y = np.zeros_like(e)
    for t in range(2, T + 200):
        y[t] = 0.5 * y[t - 1] - 0.3 * y[t - 2] + e[t]
        y[t, :, 1:] += 0.35 * y[t - 1, :, :-1]
        y[t, :, 5:] += 0.25 * y[t - 2, :, :-5]
    x = y[200:]
    m = sc.Multitaper(x, sampling_frequency=1000.0, time_halfbandwidth_product=3)
    c = sc.Connectivity.from_multitaper(m, dtype=np.complex128)
    pairs = [(0, 1), (3, 8), (10, 40), (62, 63)]
    got = c.subset_pairwise_spectral_granger_prediction(pairs)
    assert got.shape == (1, 2049, C, C) and c._last_wilson["not_converged"] == 0
    chans = sorted({ch for p in pairs for ch in p})
    pos = {ch: k for k, ch in enumerate(chans)}
    coef, _ = so.multitaper_fft(x[:, :, chans], fs=1000.0, NW=3)
    ref = so.pairwise_spectral_granger_prediction(coef, pairs=[(pos[i], pos[j]) for i, j in pairs])
    worst = 0.0
    for i, j in pairs:
        for a, b in ((i, j), (j, i)):
            g, r = got[0, :, a, b], ref[0, :, pos[a], pos[b]]
            both = ~np.isnan(g) & ~np.isnan(r)
            flip = np.isnan(g) != np.isnan(r)                      # gp <= 0 -> NaN: only a value within rounding of 0 may flip
            assert np.all(np.abs(np.where(np.isnan(g), r, g)[flip]) <= 1e-7 * np.nanmax(r))
            big = both & (np.abs(r) > 1e-3 * np.nanmax(r))
            worst = max(worst, (np.abs(g[big] - r[big]) / np.abs(r[big])).max())
            assert np.abs(g[both] - r[both]).max() <= 1e-7 * np.nanmax(r)
    print(f"  cfg4 full size, Granger: worst elementwise relative error {worst:.2e} on entries above 1e-3 of the maximum")
    assert worst < 1e-5


@pytest.mark.parametrize("C", [65, 128, 129, 256])
def test_global_coherence_large_float64(sc, C):
    """Global coherence of 65 ... 256 signals from double records (the Householder kernel global_coherence_eigh_kernel<256>; the
    packed Jacobi kernels are diagnostics, SC_GLOBAL_EIG=jacobi): squared singular values of the oracle to 1e-11, dominant vector
    as a line."""
    from oracle import spectral_oracle as so
    x = np.random.default_rng(C).standard_normal((64, 110, C))
    x[:, :, : C // 2] += np.random.default_rng(1).standard_normal((64, 110, 1))
    kw = dict(sampling_frequency=128.0, time_halfbandwidth_product=2, n_time_samples_per_window=32)
    coef, _ = so.multitaper_fft(x, fs=128.0, NW=2, n_time_samples_per_window=32)
    ref, ref_vecs = so.global_coherence(coef, max_rank=3)
    vals, vecs = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw)).global_coherence(max_rank=3)
    close64(vals, ref, rtol=1e-11, floor=1e-12, what=f"global coherence C={C}")
    ip = np.abs(np.sum(np.conj(vecs[..., -1]) * ref_vecs[..., -1], axis=-1))
    assert (ip > 1 - 1e-6).mean() > 0.9, f"C={C}: dominant vector differs ({ip.min()})"


@pytest.mark.parametrize("sizes", [(33, 40), (128, 70)])
def test_canonical_coherence_large_groups_float64(sc, sizes):
    """Canonical coherence of groups beyond 32 channels from double records: the oracle's SVD form to 1e-7."""
    from oracle import spectral_oracle as so
    C = sum(sizes)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(C)
    x = rng.standard_normal((64, 60, C)) + 0.7 * rng.standard_normal((64, 60, 1))
    kw = dict(sampling_frequency=128.0, time_halfbandwidth_product=2, n_time_samples_per_window=32)
    coef, _ = so.multitaper_fft(x, fs=128.0, NW=2, n_time_samples_per_window=32)
    ref, _ = so.canonical_coherence(coef, labels)
    got, _ = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw)).canonical_coherence(labels)
    close64(got, ref, rtol=1e-7, floor=1e-9, what=f"canonical coherence, groups {sizes}")


@pytest.mark.parametrize("case", ["ragged", "sixteen", "degenerate", "tiny", "big"])
def test_canonical_coherence_top_eigenvalue_kernel_equals_the_jacobi_kernel(sc, debug_env, case):
    """Groups of at most 16 channels: the (bin, pair) kernel reduces B = M M^H to a tridiagonal matrix by Householder reflections in
    registers and brackets its LARGEST eigenvalue by multisection on the Sturm sequence (csrc/sc_canonical.hip, round 5);
    SC_CANON_EIG=jacobi keeps the parallel Jacobi of rounds 1-4, which finds all sixteen.  Both from the same double records:
    the new kernel equals the oracle's SVD form (connectivity.py:745-820) to 1e-12, the Jacobi kernel to 1e-7 -- ragged group sizes incl.
    single channels, full groups, groups with duplicated channels (rank-deficient blocks fail the Cholesky in both: NaN pattern
    equal), and a group pair with a coupling at the rounding level.  "big" (round 6): groups beyond 32 channels, a workgroup per (bin,
    pair) -- canonical_big_hh_kernel (Householder reflections over B in LDS, lambda_max by 256-way multisection on the Sturm count)
    against canonical_big_kernel (the parallel Jacobi over the packed triangle)."""
    from oracle import spectral_oracle as so
    rng = np.random.default_rng({"ragged": 3, "sixteen": 4, "degenerate": 5, "tiny": 6, "big": 7}[case])
    sizes = {"ragged": (1, 16, 7, 2, 11, 16, 3), "sixteen": (16,) * 6, "degenerate": (8, 8, 5), "tiny": (6, 9), "big": (40, 64, 33, 100)}[case]
    C = sum(sizes)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    T, R = 128, 40
    x = rng.standard_normal((T, R, C))
    if case != "tiny":
        x += 0.8 * rng.standard_normal((T, R, 1)) + 0.5 * x[:, :, ::-1]
    if case == "degenerate":
        x[:, :, 9] = x[:, :, 8]                       # group 1 holds one channel twice
    kw = dict(sampling_frequency=128.0, time_halfbandwidth_product=2, n_time_samples_per_window=64)
    out = {}
    for eig in (None, "jacobi"):
        debug_env("SC_CANON_EIG", eig)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[eig], _ = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw)).canonical_coherence(labels)
    a, b = out[None], out["jacobi"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert ok.any()
    # (the Jacobi kernel takes its rotation angles in float32 and stops at off^2 <= 1e-24 dia^2: 1e-9 ... 1e-8 of the value; the
    #  new one sits at the rounding of the doubles)
    assert np.abs(a[ok] - b[ok]).max() <= 1e-7 * np.abs(b[ok]).max(), np.abs(a[ok] - b[ok]).max()
    if case != "degenerate":
        coef, _ = so.multitaper_fft(x, fs=128.0, NW=2, n_time_samples_per_window=64)
        ref, _ = so.canonical_coherence(coef, labels)
        close64(a, ref, rtol=1e-12, floor=1e-13, what=f"canonical coherence, groups {sizes}")
        close64(b, ref, rtol=1e-7, floor=1e-9, what=f"canonical coherence (Jacobi kernel), groups {sizes}")


def test_incremental_records_equal_fresh_ones(sc):
    """float64 engine: a measure asked for after others re-uses the record families already accumulated (copied into the
    wider record) and computes only the missing ones -- bit for bit what a fresh Connectivity returns."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((256, 30, 70))
    x[:, :, 1:] += 0.4 * x[:, :, :-1]
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=64)
    order = ["coherence_magnitude", "weighted_phase_lag_index", "phase_locking_value", "debiased_squared_weighted_phase_lag_index",
             "phase_lag_index", "power", "pairwise_phase_consistency"]
    c = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw))
    for name in order:
        got = getattr(c, name)()
        fresh = getattr(sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw)), name)()
        assert np.array_equal(np.nan_to_num(got, nan=-7.0), np.nan_to_num(fresh, nan=-7.0)), name
    ints = [k for k in c._accum_cache if isinstance(k, int)]
    union = 0
    for k in ints:
        assert union & k == 0, ints                 # no family is held (or was computed) twice
        union |= k
    assert bin(union).count("1") == 5, ints


@pytest.mark.parametrize("L", [64, 128, 256, 512, 1024])
def test_radix16_float64_transform_equals_the_wave_per_pair_kernel_and_the_oracle(sc, debug_env, L):
    """Powers of two 64 ... 1024 take the register-resident radix-16 kernel in doubles (round 3); SC_MTFFT_F64=wave keeps the
    radix-4 wave-per-pair kernel reachable: both against the oracle (1e-11 of the maximum) and against each other."""
    from oracle import spectral_oracle as so
    rng = np.random.default_rng(L)
    C = 11 if L == 256 else 6                       # an odd channel count once: unpaired last channel
    x = rng.standard_normal((L + L // 2, 3, C)) + np.linspace(0, 2, L + L // 2)[:, None, None]
    kw = dict(sampling_frequency=500.0, time_halfbandwidth_product=3, n_time_samples_per_window=L, n_time_samples_per_step=L // 2,
              detrend_type="linear")
    got = sc.Multitaper(x, **kw).fft()
    ref, _ = so.multitaper_fft(x, fs=500.0, NW=3, n_time_samples_per_window=L, n_time_samples_per_step=L // 2, detrend_type="linear")
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-11 * scale
    debug_env("SC_MTFFT_F64", "wave")
    wave = sc.Multitaper(x, **kw).fft()
    assert np.abs(wave - got).max() <= 1e-12 * scale
