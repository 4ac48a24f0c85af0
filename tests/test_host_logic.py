"""Host-side mirror of the reference API: derived parameters, tapers, validation messages.
Expected values are golden vectors produced by the real reference (oracle/gen_golden.py);
the error/warning regexes are the ones the reference's own tests match
(reference tests/test_transforms.py:338-586, tests/test_connectivity.py:855-895)."""
import warnings

import numpy as np
import pytest

from spectral_connectivity_amd import Connectivity, Multitaper, estimate_n_tapers, prepare_time_series
from spectral_connectivity_amd.transforms import dpss_windows


def test_geometry_matches_reference(golden):
    g = golden("f4_lengths")
    x = g["x"]
    cases = {
        "L250": dict(n_time_samples_per_window=250),
        "L250_N300": dict(n_time_samples_per_window=250, n_fft_samples=300),
        "L255": dict(n_time_samples_per_window=255),
        "L256_N255": dict(n_time_samples_per_window=256, n_fft_samples=255),
        "dur_step": dict(time_window_duration=0.8, time_window_step=0.29),
    }
    for tag, kw in cases.items():
        m = Multitaper(x, sampling_frequency=250.0, time_halfbandwidth_product=2, **kw)
        np.testing.assert_allclose(m.time, g[f"{tag}__time"], rtol=1e-12)
        np.testing.assert_allclose(m.frequencies, g[f"{tag}__frequencies"], rtol=1e-12)
        assert m.n_fft_samples == g[f"{tag}__fft"].shape[3]
        assert m.n_time_windows == g[f"{tag}__fft"].shape[0]
        c = Connectivity(np.zeros((1, 1, 1, m.n_fft_samples, 2), complex), frequencies=m.frequencies)
        np.testing.assert_allclose(c.frequencies, g[f"{tag}__conn_frequencies"], rtol=1e-12)


def test_step_truncation_quirk():
    # int(0.29*100) == 28: the reference truncates the step but rounds the window
    m = Multitaper(np.zeros((1000, 1, 1)), sampling_frequency=100, time_window_duration=0.5,
                   time_window_step=0.29)
    assert m.n_time_samples_per_step == 28 and m.n_time_samples_per_window == 50


@pytest.mark.parametrize("L,NW", [(1024, 3.0), (256, 4.0), (4096, 3.0), (250, 2.0), (64, 2.5)])
def test_dpss_matches_reference(golden, L, NW):
    g = golden("f8_dpss")
    tapers, eig = dpss_windows(L, NW, int(np.floor(2 * NW - 1)), is_low_bias=False)
    np.testing.assert_allclose(tapers, g[f"L{L}_NW{NW}__tapers"], rtol=1e-7, atol=1e-11)
    np.testing.assert_allclose(eig, g[f"L{L}_NW{NW}__eig"], rtol=1e-9)


def test_tapers_property_and_low_bias(golden):
    g = golden("f7_edges")
    x = g["nw175__x"]
    m = Multitaper(x, sampling_frequency=100.0, time_halfbandwidth_product=1.75)
    np.testing.assert_allclose(m.tapers, g["nw175__tapers"], atol=1e-10)
    m = Multitaper(x, sampling_frequency=100.0, time_halfbandwidth_product=1.0)
    np.testing.assert_allclose(m.tapers, g["nw1__tapers"], atol=1e-10)
    # reference tests/test_transforms.py:62-71
    assert [estimate_n_tapers(nw) for nw in (3, 1, 1.75)] == [5, 1, 2]
    assert Multitaper(x, time_halfbandwidth_product=3).n_tapers == 5


def test_multitaper_validation_messages():
    with pytest.raises(ValueError, match=r"Expected 3D array.*got 1D"):
        Multitaper(np.zeros(10))
    with pytest.raises(ValueError, match=r"Expected 3D array.*got 2D"):
        Multitaper(np.zeros((10, 2)))
    with pytest.raises(ValueError, match=r"Expected 3D array.*got 4D"):
        Multitaper(np.zeros((10, 2, 2, 2)))
    x = np.zeros((100, 2, 2))
    with pytest.raises(ValueError, match=r"sampling_frequency.*must be positive"):
        Multitaper(x, sampling_frequency=0)
    with pytest.raises(ValueError, match=r"time_halfbandwidth_product.*must be at least 1"):
        Multitaper(x, time_halfbandwidth_product=0.5)
    with pytest.raises(ValueError, match=r"time_window_duration.*must be positive"):
        Multitaper(x, time_window_duration=-1)
    with pytest.raises(ValueError, match=r"time_window_step.*must be positive"):
        Multitaper(x, time_window_step=0)
    with pytest.warns(UserWarning, match=r"data may be transposed"):
        Multitaper(np.zeros((5, 1, 10)))
    bad = x.copy()
    bad[3, 0, 0] = np.nan
    with pytest.warns(UserWarning, match=r"contains NaN.*infinite values"):
        Multitaper(bad)
    with pytest.warns(UserWarning, match=r"unusually large"):
        Multitaper(x, time_halfbandwidth_product=11)
    with pytest.warns(UserWarning, match=r"creates gaps"):
        Multitaper(x, sampling_frequency=100, time_window_duration=0.1, time_window_step=0.2)


def test_prepare_time_series():
    assert prepare_time_series(np.zeros(7)).shape == (7, 1, 1)
    assert prepare_time_series(np.zeros((7, 3)), axis="signals").shape == (7, 1, 3)
    assert prepare_time_series(np.zeros((7, 3)), axis="trials").shape == (7, 3, 1)
    with pytest.raises(ValueError, match=r"For 2D input.*must specify.*axis.*parameter"):
        prepare_time_series(np.zeros((7, 3)))
    with pytest.raises(ValueError, match=r"axis must be.*'signals'.*'trials'"):
        prepare_time_series(np.zeros((7, 3)), axis="x")


def test_connectivity_validation_messages():
    for nd in (1, 2, 3, 4, 6):
        with pytest.raises(ValueError, match=f"must be 5-dimensional, got {nd}D"):
            Connectivity(np.zeros((2,) * nd, complex))
    with pytest.raises(ValueError, match=r"Expected shape.*n_time_windows.*n_trials.*n_tapers"):
        Connectivity(np.zeros((2, 2), complex))
    with pytest.raises(ValueError, match="use the Multitaper class"):
        Connectivity(np.zeros((2, 2), complex))
    with pytest.raises(ValueError, match=r"Did you mean 'trials_tapers'"):
        Connectivity(np.zeros((1, 1, 1, 4, 2), complex), expectation_type="tapers_trials")
    coef = np.zeros((1, 1, 1, 4, 2), complex)
    coef[0, 0, 0, 0, 0] = np.inf
    with pytest.warns(UserWarning, match="NaN or Inf"):
        Connectivity(coef)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c = Connectivity(np.ones((3, 5, 7, 8, 2), complex), expectation_type="time_tapers")
    assert c.n_observations == 21


def test_parameter_helpers_match_reference_values():
    """Expected dicts were produced by the real reference (reference transforms.py:199-402)."""
    from spectral_connectivity_amd import suggest_parameters
    assert suggest_parameters(1000, 10.0) == {
        "sampling_frequency": 1000, "time_halfbandwidth_product": 3.0, "time_window_duration": 2.0,
        "n_tapers": 5, "frequency_resolution": 3.0, "n_time_windows": 5, "nyquist_frequency": 500.0}
    p = suggest_parameters(500, 60.0, desired_n_tapers=9)
    assert (p["time_halfbandwidth_product"], p["n_tapers"], p["time_window_duration"]) == (5.0, 9, 12.0)
    p = suggest_parameters(1000, 3.0, desired_freq_resolution=3.0)      # window capped at a third of the signal
    assert p["time_window_duration"] == 1.0 and p["time_halfbandwidth_product"] == 1.5 and p["n_time_windows"] == 3
    with pytest.raises(ValueError, match="Cannot achieve desired frequency resolution"):
        suggest_parameters(250, 2.0, desired_freq_resolution=0.5)
    with pytest.warns(UserWarning, match="Both 'desired_freq_resolution' and 'desired_n_tapers'"):
        suggest_parameters(1000, 10.0, desired_freq_resolution=2.0, desired_n_tapers=3)
    m = Multitaper(np.zeros((5000, 1, 64)), sampling_frequency=1000, time_window_duration=1.0,
                   time_halfbandwidth_product=3)
    text = m.summarize_parameters()
    for line in ("Time samples:    5000 (5.00 seconds)", "Number of tapers:              5",
                 "Window step:      1.000 s (non-overlapping)", "Number of windows: 5",
                 "Frequency resolution: 6.0 Hz", "FFT samples:          1000"):
        assert line in text, line


# ---- band post-processing of the coherency and the statistics helpers (host-side NumPy) ------------------
def test_phase_slope_index_and_delay_match_reference(golden):
    from spectral_connectivity_amd import _postprocess as pp
    g = golden("f11_post")
    coh, f, res = g["coherency"], g["frequencies"], float(g["frequency_resolution"])
    np.testing.assert_allclose(pp.phase_slope_index(coh, f), g["psi_all"], rtol=1e-9, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(pp.phase_slope_index(coh, f, [10, 200]), g["psi_band"], rtol=1e-9, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(pp.phase_slope_index(coh, f, [10, 200], res), g["psi_band_res"], rtol=1e-9, atol=1e-9,
                               equal_nan=True)
    # delay(): the reference's output is the constant 2 pi k for every frequency and pair (raw data of a fully
    # masked array, because its one-sample z-score is always NaN) -- reproduced by default
    ref = g["delay_band"]
    np.testing.assert_allclose(ref[0, :, :, 0, 1], np.broadcast_to(2 * np.pi * np.arange(-2, 3), ref.shape[1:3]))
    got = pp.delay(coh, f, int(g["n_observations"]), [10, 200], n_range=2)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True)
    d, s_, r = pp.group_delay(coh, f, int(g["n_observations"]), [10, 200], res)
    for a, b in ((d, g["group_delay"]), (s_, g["group_slope"]), (r, g["group_r"])):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)


@pytest.fixture
def unbiased_one_sample_z():
    from spectral_connectivity_amd import options
    options.one_sample_fisher_z = "unbiased"
    yield
    options.one_sample_fisher_z = "reference"


def test_delay_with_the_unbiased_one_sample_z(golden, unbiased_one_sample_z):
    """options.one_sample_fisher_z = "unbiased": delay() carries the candidates (phase + 2 pi k) / 2 pi at the
    significant frequencies and NaN elsewhere."""
    from spectral_connectivity_amd import _postprocess as pp
    g = golden("f11_post")
    coh, f = g["coherency"], g["frequencies"]
    got = pp.delay(coh, f, int(g["n_observations"]), [10, 200], n_range=2)
    assert got.shape == g["delay_band"].shape
    band = f[(f > 10) & (f < 200)]
    k0 = got[0, :, 2, 0, 1]                      # k = 0 candidate, pair (0, 1): phase / 2 pi = f * tau
    ok = ~np.isnan(k0)
    assert ok.sum() >= 20
    assert abs(np.median(k0[ok] / band[ok]) - 0.010) < 3e-4 and np.abs(k0[ok] / band[ok] - 0.010).max() < 6e-3
    np.testing.assert_allclose(got[0, :, 3, 0, 1][ok] - k0[ok], 1.0)
    np.testing.assert_allclose(got[0, :, :, 1, 0], -got[0, :, :, 0, 1], equal_nan=True)


def test_group_delay_recovers_a_known_delay(golden, unbiased_one_sample_z):
    """Channel 1 is channel 0 delayed by 5 samples at 500 Hz.  The reference's own group_delay() returns NaN
    for every pair (its one-sample Fisher z evaluates coherence_bias(0) = -1/2 and takes the square root of a
    negative number, so no frequency is ever significant) -- the default here as well; with
    options.one_sample_fisher_z = "unbiased" the regression recovers the delay."""
    from spectral_connectivity_amd import _postprocess as pp
    g = golden("f11_post")
    assert np.isnan(g["group_delay"][0, 0, 1]) and np.isnan(g["group_r"][0, 0, 1]) and g["group_r"][0, 0, 0] == 1.0
    d, s, r = pp.group_delay(g["coherency"], g["frequencies"], int(g["n_observations"]), [10, 200],
                             float(g["frequency_resolution"]))
    assert d.shape == g["group_delay"].shape
    assert abs(d[0, 0, 1] - 0.010) < 2e-4 and abs(d[0, 1, 0] + 0.010) < 2e-4
    assert r[0, 0, 1] > 0.999 and r[0, 0, 0] == 1.0 and np.isnan(s[0, 0, 0])
    np.testing.assert_allclose(s, 2 * np.pi * d, equal_nan=True)
    # a pair of independent channels has no significant run: NaN
    assert np.isnan(d[0, 0, 2]) or abs(r[0, 0, 2]) <= 1.0


def test_statistics_helpers_match_reference(golden):
    from spectral_connectivity_amd import statistics as st
    g = golden("f11_post")
    p = g["stat_p"]
    np.testing.assert_array_equal(st.Benjamini_Hochberg_procedure(p, alpha=0.05), g["stat_bh"])
    np.testing.assert_array_equal(st.Benjamini_Hochberg_procedure(0.5 + 0.5 * p, alpha=0.01), g["stat_bh_none"])
    np.testing.assert_array_equal(st.Bonferroni_correction(p, alpha=0.05), g["stat_bonf"])
    np.testing.assert_array_equal(st.adjust_for_multiple_comparisons(p, method="Bonferroni_correction"), g["stat_bonf"])
    z = st.coherence_fisher_z_transform(g["stat_coh1"], 40, g["stat_coh2"], 25)
    np.testing.assert_allclose(z, g["stat_fisher2"], rtol=1e-12)
    np.testing.assert_allclose(st.get_normal_distribution_p_values(z), g["stat_pvals"], rtol=1e-12)
    assert st.coherence_bias(40) == float(g["stat_coh_bias"])
    np.testing.assert_allclose(st.coherence_rate_adjustment(10.0, 14.0, np.linspace(0.5, 3, 6), 0.2, 0.5),
                               g["stat_rate_adj"], rtol=1e-12)
    lo, hi = st.power_confidence_intervals(7, power=np.linspace(1, 4, 5), ci=0.9)
    np.testing.assert_allclose(lo, g["stat_ci_lo"], rtol=1e-12)
    np.testing.assert_allclose(hi, g["stat_ci_hi"], rtol=1e-12)
    np.testing.assert_allclose(st.power_bias(35), g["stat_power_bias"], rtol=1e-12)
    np.testing.assert_allclose(st.power_variance(35), g["stat_power_var"], rtol=1e-12)
    np.testing.assert_allclose(st.power_fisher_z_transform(np.linspace(1, 4, 5), 35, np.linspace(2, 3, 5), 21),
                               g["stat_power_z"], rtol=1e-12)
    # one-sample z-score: NaN like the reference's by default, finite with the unbiased option
    from spectral_connectivity_amd import options
    assert np.isnan(st.coherence_fisher_z_transform(g["stat_coh1"], 40)).all()
    options.one_sample_fisher_z = "unbiased"
    try:
        assert np.isfinite(st.coherence_fisher_z_transform(g["stat_coh1"], 40)).all()
    finally:
        options.one_sample_fisher_z = "reference"


def test_wrapper_validates_before_touching_the_device():
    """Methods the labelled interface cannot express are refused with the reference's message (wrapper.py:71-78)
    -- before xarray or the GPU are needed."""
    from spectral_connectivity_amd import multitaper_connectivity
    from spectral_connectivity_amd.wrapper import connectivity_to_xarray
    x = np.random.default_rng(0).standard_normal((64, 2, 2))
    for bad in ("group_delay", "canonical_coherence", "directed_transfer_function", "partial_directed_coherence"):
        with pytest.raises(ValueError, match="not supported by the xarray interface"):
            multitaper_connectivity(x, sampling_frequency=100, method=bad)
        with pytest.raises(ValueError, match="Connectivity class directly"):
            connectivity_to_xarray(Multitaper(x, sampling_frequency=100), method=bad)


def test_vendored_labelled_arrays():
    """_labelled.DataArray / Dataset: what the front end returns when the optional xarray package is absent."""
    from spectral_connectivity_amd._labelled import DataArray, Dataset
    v = np.arange(2 * 3 * 2 * 2, dtype=float).reshape(2, 3, 2, 2)
    a = DataArray(v, coords=[[0.0, 0.5], [0.0, 10.0, 20.0], ["a", "b"], ["a", "b"]],
                  dims=["time", "frequency", "source", "target"], name="coherence_magnitude", attrs={"mt_n_tapers": 5})
    assert a.dims == ("time", "frequency", "source", "target") and a.shape == (2, 3, 2, 2) and a.name == "coherence_magnitude"
    np.testing.assert_array_equal(a["frequency"], [0.0, 10.0, 20.0])
    np.testing.assert_array_equal(a.sel(source="a", target="b").values, v[:, :, 0, 1])
    assert a.sel(source="a", target="b").dims == ("time", "frequency")
    np.testing.assert_array_equal(a.sel(frequency=12.0, method="nearest").values, v[:, 1])
    np.testing.assert_array_equal(a.isel(time=1, frequency=[0, 2]).values, v[1][[0, 2]])
    assert a.isel(time=[0]).squeeze().dims == ("frequency", "source", "target")
    np.testing.assert_array_equal(np.asarray(a), v)
    with pytest.raises(KeyError):
        a.sel(source="zz")
    with pytest.raises(ValueError, match="coordinate 'frequency'"):
        DataArray(v, coords=[[0, 1], [0, 1], ["a", "b"], ["a", "b"]], dims=["time", "frequency", "source", "target"])
    ds = Dataset()
    ds["coherence_magnitude"] = a
    assert list(ds) == ["coherence_magnitude"] and ds.data_vars is ds and ds.attrs == {"mt_n_tapers": 5}


def test_host_detrend_helper_matches_scipy_and_reference_messages():
    """transforms.detrend (reference transforms.py:1798-1915, a restatement of scipy.signal.detrend)."""
    import scipy.signal
    from spectral_connectivity_amd.transforms import detrend
    x = np.random.default_rng(0).standard_normal((50, 3, 7)) + np.linspace(0, 5, 50)[:, None, None]
    for kw in (dict(axis=0), dict(axis=0, bp=[20, 35]), dict(axis=0, type="constant"), dict(axis=-1), dict(axis=1, type="l")):
        np.testing.assert_allclose(detrend(x, **kw), scipy.signal.detrend(x, **kw), atol=1e-12)
    with pytest.raises(ValueError, match="Invalid trend type 'cubic' is not supported"):
        detrend(x, type="cubic")
    with pytest.raises(ValueError, match="exceed data length"):
        detrend(np.zeros(100), type="linear", bp=[150])


def test_simulate_mvar_reproduces_a_known_var_process():
    """simulate.simulate_MVAR: shape contract, determinism in the seed, and the lag-1 cross-covariance of a stable
    VAR(1) (Gamma_1 = A Gamma_0) on a long realisation."""
    from spectral_connectivity_amd.simulate import simulate_MVAR
    A = np.array([[[0.5, 0.2], [-0.1, 0.4]]])
    x = simulate_MVAR(A, n_time_samples=20000, n_trials=2, n_burnin_samples=200, random_state=1)
    assert x.shape == (20000, 2, 2)
    np.testing.assert_array_equal(x, simulate_MVAR(A, n_time_samples=20000, n_trials=2, n_burnin_samples=200,
                                                   random_state=np.random.default_rng(1)))
    z = x[:, 0]
    g0 = z[:-1].T @ z[:-1] / (len(z) - 1)
    g1 = z[1:].T @ z[:-1] / (len(z) - 1)
    np.testing.assert_allclose(g1, A[0] @ g0, atol=0.05)


def test_dpss_interpolated_from_a_shorter_window():
    """dpss_windows(interp_from=...): tapers of the short length, interpolated and renormalised (transforms.py:1615-1651);
    they stay close to the directly computed ones, keep unit norm and the sign conventions."""
    direct, eig = dpss_windows(256, 3, 5, is_low_bias=False)
    interp, eig_i = dpss_windows(256, 3, 5, is_low_bias=False, interp_from=64, interp_kind="cubic")
    assert interp.shape == direct.shape
    np.testing.assert_allclose(np.linalg.norm(interp, axis=1), 1.0, atol=1e-12)
    assert np.abs(interp - direct).max() < 2e-2 and np.abs(eig - eig_i).max() < 2e-2     # the grid is shifted (endpoint=False)
    assert (interp[::2].sum(axis=1) > 0).all()


def test_tridiagonal_helpers():
    """tridisolve / tridi_inverse_iteration (reference transforms.py:1443-1536): solve and eigenvector of a symmetric
    tridiagonal matrix, checked against dense linear algebra."""
    from spectral_connectivity_amd.transforms import tridi_inverse_iteration, tridisolve
    rng = np.random.default_rng(0)
    d, e, b = rng.uniform(2, 3, 9), rng.uniform(-0.5, 0.5, 8), rng.standard_normal(9)
    A = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    np.testing.assert_allclose(tridisolve(d, e, b.copy()), np.linalg.solve(A, b), rtol=1e-12)
    keep = b.copy()
    out = tridisolve(d, e, keep, overwrite_b=False)
    np.testing.assert_array_equal(keep, b)
    np.testing.assert_allclose(out, np.linalg.solve(A, b), rtol=1e-12)
    w, V = np.linalg.eigh(A)
    v = tridi_inverse_iteration(d, e, w[-1] + 1e-9, x0=np.ones(9))
    assert abs(abs(v @ V[:, -1]) - 1.0) < 1e-8 and abs(np.linalg.norm(v) - 1.0) < 1e-12


def test_public_api_surface_matches_the_reference():
    """Every public function, class, method / property and module constant of the reference exists here with the same
    argument names, order and default values (tests/golden/api_surface.json, generated from the reference by
    oracle/gen_golden.py api).  Only private helpers differ."""
    import ast
    import json
    import os
    import spectral_connectivity_amd as pkg
    root = os.path.dirname(pkg.__file__)
    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "api_surface.json")))
    assert set(ref["__all__"]) <= set(pkg.__all__)

    def describe(fn):
        a = fn.args
        pos = a.posonlyargs + a.args
        dflt = [None] * (len(pos) - len(a.defaults)) + [ast.unparse(x) for x in a.defaults]
        args = [[p.arg, d] for p, d in zip(pos, dflt)]
        args += [[k.arg, ast.unparse(v) if v is not None else None] for k, v in zip(a.kwonlyargs, a.kw_defaults)]
        return args

    problems = []
    for module, names in ref.items():
        if module == "__all__":
            continue
        path = os.path.join(root, module + ".py")
        assert os.path.exists(path), f"module {module} missing"
        tree = ast.parse(open(path).read())
        have = {}
        for n in tree.body:
            if isinstance(n, ast.FunctionDef):
                have[n.name] = describe(n)
            elif isinstance(n, ast.ClassDef):
                for m in n.body:
                    if isinstance(m, ast.FunctionDef):
                        have[n.name + "." + m.name] = describe(m)
            elif isinstance(n, ast.Assign):
                for tg in n.targets:
                    if isinstance(tg, ast.Name):
                        have[tg.id] = ast.unparse(n.value)
        for name, spec in names.items():
            if name not in have:
                problems.append(f"{module}.{name} missing")
            elif "constant" in spec:
                if name == "TIKHONOV_REGULARIZATION_FACTOR":
                    assert float(have[name]) == float(spec["constant"])
            else:
                mine = [[a, (d or "").replace("np.", "xp.") or None] for a, d in have[name]]
                want = [[a, (d or "").replace("np.", "xp.") or None] for a, d in spec["args"]]
                if mine != want:
                    problems.append(f"{module}.{name}: {mine} != {want}")
    assert not problems, "\\n".join(problems)


@pytest.mark.parametrize("n_signals", [257, 300, 306, 384, 385, 512, 1024])
def test_tile_plan_covers_the_full_record_once(n_signals):
    """_lib.tile_plan (the channel-block tiling of more than 256 signals, both hosts): over all block pairs every tile of the full
    record is written exactly once, and every (src, dst) names the same 16 x 16 channel tile -- recomputed here from the pair's
    channel columns, not through the plan's own index arithmetic."""
    from spectral_connectivity_amd import _lib
    NB = -(-n_signals // 16)
    written = []
    for a, b, cols, src, dst in _lib.tile_plan(n_signals):
        assert a < b and len(cols) <= 256 and len(src) == len(dst)
        nb_s = -(-len(cols) // 16)
        upper = [(ti, tj) for ti in range(nb_s) for tj in range(ti, nb_s)]          # tile index -> (row, column) of the pair's record
        for s, d in zip(src, dst):
            ti, tj = upper[s]
            gi, gj = cols[16 * ti] // 16, cols[16 * tj] // 16
            assert gi <= gj
            assert d == sum(NB - r for r in range(gi)) + (gj - gi), (n_signals, a, b, s, d)
        written += list(dst)
    assert sorted(written) == list(range(NB * (NB + 1) // 2))


def test_blockwise_granger_call_sequence(monkeypatch):
    """_stage_d.blockwise_granger against a library stub that records its arguments, on plain NumPy memory: two batch sizes m of
    three pairs each under a bound of two pairs per call -- calls of (2, 1, 2, 1) pairs, the output kept on every call but the
    first, the list and n_iter / status pointers advanced per chunk, the summaries combined as max, sum, sum."""
    import ctypes

    from spectral_connectivity_amd import _lib, _stage_d

    class Memory:
        def empty(self, shape, dtype):
            return np.empty(shape, dtype)

        zeros = staticmethod(np.zeros)
        upload = staticmethod(np.array)

        def ptr(self, a, first_row=0):
            return ctypes.c_void_p(a.ctypes.data + first_row * (a.strides[0] if a.ndim else 0))

        def stream(self):
            return None

        def is_f64(self, record):
            return record.dtype == np.float64

        def fill_nan(self, a):
            a.fill(np.nan)

    class Library:
        calls = []

        @staticmethod
        def sc_blockwise_granger_workspace_bytes(n_groups, m, n_fft, n, nbytes):
            nbytes._obj.value = 1000 + 100 * n
            return 0

        @classmethod
        def sc_blockwise_granger_f64(cls, accum, spectra, n_groups, n_freq, n_fft, n_signals, planes, n_obs, members, split, cell, n, m,
                                     n_blocks, tolerance, max_iterations, work, nbytes, flags, out, n_iter, status, summary, stream):
            cls.calls.append(dict(n=n, m=m, flags=flags, planes=planes, nbytes=nbytes, members=members.value, split=split.value,
                                  cell=cell.value, out=out.value, n_iter=n_iter.value, status=status.value))
            summary[0], summary[1], summary[2] = 10 * len(cls.calls), len(cls.calls), 2
            return 0

    monkeypatch.setattr(_lib, "_lib", Library)
    monkeypatch.setattr(_lib, "CONDITIONAL_WORK_BYTES", 1000 + 100 * 2)
    n_groups, held = 3, []
    mem = Memory()
    mem.upload = lambda a: held.append(np.array(a)) or held[-1]          # (the test reads the uploaded arrays' addresses)
    mem.zeros = lambda shape, dtype: held.append(np.zeros(shape, dtype)) or held[-1]
    batches = {m: (np.zeros((3, m), np.int32), np.zeros(3, np.int32), np.zeros((3, 2), np.int32)) for m in (3, 4)}
    accum = np.zeros((n_groups * 5, 8), np.float64)
    out, n_iter, status, summary = _stage_d.blockwise_granger(mem, n_groups, 8, 7, batches, 4, accum=accum, n_freq_accum=5,
                                                              planes=_lib.PLANE_CSM, n_obs=9)
    calls = Library.calls
    assert [c["n"] for c in calls] == [2, 1, 2, 1] and [c["m"] for c in calls] == [3, 3, 4, 4]
    assert [c["flags"] for c in calls] == [0] + [_lib.BLOCKWISE_KEEP_OUTPUT] * 3
    assert all(c["planes"] == _lib.PLANE_CSM | _lib.RECORD_F64 and c["nbytes"] == 1200 and c["out"] == out.ctypes.data for c in calls)
    d_n_iter, d_status = held[0], held[1]
    assert n_iter is d_n_iter and status is d_status and n_iter.shape == (6, n_groups) and out.shape == (n_groups, 5, 4, 4)
    for k, c in enumerate(calls):
        members, split, cell = held[2 + 3 * (k // 2):5 + 3 * (k // 2)]
        q0, row, m = 2 * (k % 2), 3 * (k // 2), c["m"]
        assert c["members"] == members.ctypes.data + 4 * q0 * m
        assert c["split"] == split.ctypes.data + 4 * q0
        assert c["cell"] == cell.ctypes.data + 8 * q0
        assert c["n_iter"] == d_n_iter.ctypes.data + 4 * (row + q0) * n_groups
        assert c["status"] == d_status.ctypes.data + 4 * (row + q0) * n_groups
    assert summary == (40, 1 + 2 + 3 + 4, 8)
    # no batch at all (every pair rank deficient): no call, the output NaN-filled by the host
    del calls[:]
    out, n_iter, status, summary = _stage_d.blockwise_granger(mem, n_groups, 8, 7, {}, 4, accum=accum, n_freq_accum=5,
                                                              planes=_lib.PLANE_CSM, n_obs=9)
    assert not calls and np.isnan(out).all() and n_iter.shape == (0, n_groups) and summary == (0, 0, 0)


def test_max_iterations_is_checked_by_every_stage_d_path():
    from spectral_connectivity_amd import _stage_d, engine
    assert engine.check_max_iterations is _stage_d.check_max_iterations
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="max_iterations must be between 1 and 1024"):
            _stage_d.check_max_iterations(bad)
    assert _stage_d.check_max_iterations(60) == 60


class _RecordingLibrary:
    """A stand-in for libsc_hip.so under the drivers of _stage_abc.py: every entry point returns 0 (or what ``answers`` names) and
    logs (name, arguments) after checking the argument count against ``_lib.SYMBOLS``; a SpectraDesc passed by reference is logged as ("desc", n_signals, n_freq)."""

    def __init__(self, **answers):
        self.answers, self.calls = answers, []

    def __getattr__(self, name):
        def entry(*args):
            from spectral_connectivity_amd import _lib
            assert len(args) == len(_lib.SYMBOLS[name][1]), f"{name}: {len(args)} arguments, the ABI has {len(_lib.SYMBOLS[name][1])}"
            seen = tuple(("desc", a._obj.n_signals, a._obj.n_freq) if hasattr(getattr(a, "_obj", None), "n_signals") else
                         getattr(a, "value", a) for a in args)
            self.calls.append((name, seen))
            answer = self.answers.get(name, 0)
            return answer(*args) if callable(answer) else answer
        return entry

    def names(self, *skip):
        return [name for name, _ in self.calls if name not in skip]

    def args(self, name):
        return [a for n, a in self.calls if n == name]


def _numpy_memory(dummy_above=1 << 22):
    import contextlib
    import ctypes

    from spectral_connectivity_amd import _stage_abc

    class Memory:
        plans, workspaces = [], []

        def empty(self, shape, dtype):
            big = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize > dummy_above
            return np.empty((1,) if big else shape, dtype)          # (only its address is taken)

        def ptr(self, a, first_row=0):
            return ctypes.c_void_p(a.ctypes.data + first_row * (a.strides[0] if a.ndim else 0))

        def stream(self):
            return None

        def is_f64(self, record):
            return record.dtype == np.float64

        def head(self, a, n):
            return a[:n]

        def twiddles(self, n_fft):
            return np.empty(n_fft, np.complex64)

        def workspace(self, n_bytes, owner=None):
            self.workspaces.append(np.empty(n_bytes, np.uint8) if n_bytes > 0 else None)
            return self.workspaces[-1]

        @contextlib.contextmanager
        def fft_plan(self, n_fft, batch, f64=False):
            self.plans.append((n_fft, batch, f64))
            yield 77

        def spectra(self, X, dims, strides, n_fft, real_input, C_alloc=None, P=None, scale=None):
            return _stage_abc.Spectra(X, dims, strides, n_fft, real_input, C_alloc, P, scale,
                                      f64=X is not None and X.dtype == np.complex128)

    return Memory()


def test_stage_a_call_sequences(monkeypatch):
    """_stage_abc.spectra_f32 / spectra_f64 against the recording library on plain NumPy memory: which entry points run, in which
    order and with which sizes, for the planes format, the fused transforms and the tapered-windows + rocFFT fallbacks."""
    from spectral_connectivity_amd import _lib, _stage_abc
    T, R, K, C, Ca, L, step, N = 64, 2, 2, 3, 4, 32, 16, 32
    W, F = 3, 17
    x, h = np.zeros((T, R, Ca), np.float32), np.zeros((K, L), np.float32)
    queries = ("sc_multitaper_fft_supported", "sc_multitaper_fft_planes_supported", "sc_planes_row_bytes", "sc_multitaper_fft_f64_supported")

    def run(fn, *args, env=None, **answers):
        kw = {k: answers.pop(k) for k in list(answers) if not k.startswith("sc_")}
        lib, mem = _RecordingLibrary(**answers), _numpy_memory()
        monkeypatch.setattr(_lib, "_lib", lib)
        monkeypatch.delenv("SC_PLANES_FORMAT", raising=False)
        monkeypatch.delenv("SC_PLANES_MIN_CHANNELS", raising=False)
        if env:
            monkeypatch.setenv("SC_PLANES_MIN_CHANNELS", env)
        return lib, mem, fn(mem, *args, **kw)

    f32_args = (x, h, T, R, Ca, C, L, step, W, N, _lib.DETREND["constant"])
    cross = _lib.PLANE_CSM | _lib.PLANE_ABS_IM
    # planes format: work-buffer size from the query, the scan, then the transform; quality still on the device
    lib, mem, sp = run(_stage_abc.spectra_f32, *f32_args, cross, env="2", taper_norms=lambda: (1.5, 0.25), sc_multitaper_fft_supported=1,
                       sc_multitaper_fft_planes_supported=1, sc_planes_row_bytes=24, sc_planes_scales_work_bytes=96)
    assert lib.names(*queries) == ["sc_planes_scales_work_bytes", "sc_planes_scales_quality_f32", "sc_multitaper_fft_planes_f32"]
    assert lib.args("sc_planes_scales_work_bytes") == [(T * R, Ca)]
    scan = lib.args("sc_planes_scales_quality_f32")[0]
    assert scan[1:6] == (T, R, Ca, 1, 1.5) and scan[8] == 96 and scan[9] == sp.quality.ctypes.data
    assert lib.args("sc_multitaper_fft_planes_f32")[0][1:8] == (T, R, Ca, L, step, W, N)
    assert sp.X is None and sp.P.nbytes == F * W * R * K * 24 and sp.scale.shape == (2 * Ca,) and sp.taper_l2_min == 0.25
    assert (sp.F, sp.W, sp.R, sp.K, sp.C, sp.C_alloc, sp.n_fft, sp.strides) == (F, W, R, K, C, Ca, N, (W * R * K * Ca, R * K * Ca, K * Ca, Ca))
    # the same request without the format's size / channel thresholds lifted, and without a hint: fused complex64
    for hint in (cross, None):
        lib, mem, sp = run(_stage_abc.spectra_f32, *f32_args, hint, sc_multitaper_fft_supported=1, sc_multitaper_fft_planes_supported=1)
        assert lib.names(*queries) == ["sc_multitaper_fft_f32"] and sp.P is None and sp.quality is None
        assert lib.args("sc_multitaper_fft_f32")[0][1:8] == (T, R, Ca, L, step, W, N) and lib.args("sc_multitaper_fft_f32")[0][12] == sp.X.ctypes.data
        assert sp.X.shape == (F, W, R, K, Ca) and sp.X.dtype == np.complex64 and not sp.f64
    # a length the fused kernel does not take: tapered windows, then the FFT through the adapter's plan
    lib, mem, sp = run(_stage_abc.spectra_f32, *f32_args, cross, env="2", sc_multitaper_fft_supported=0, sc_multitaper_fft_planes_supported=1)
    assert lib.names(*queries) == ["sc_taper_windows_f32", "sc_fft_execute"] and mem.plans == [(N, W * R * K * Ca, False)]
    assert lib.args("sc_fft_execute")[0][0] == 77 and lib.args("sc_fft_execute")[0][2] == sp.X.ctypes.data
    # float64 engine: the fused kernel; beyond 65535 trials the fallback although the kernel has the length (no such array is made)
    x64, h64 = np.zeros((T, R, C)), np.zeros((K, L))
    lib, mem, sp = run(_stage_abc.spectra_f64, x64, h64, T, R, C, L, step, W, N, 2, sc_multitaper_fft_f64_supported=1)
    assert lib.names(*queries) == ["sc_multitaper_fft_f64"] and sp.f64 and sp.X.shape == (F, W, R, K, C) and sp.C_alloc == C
    lib, mem, sp = run(_stage_abc.spectra_f64, x64[:, :1], h64, T, 65536, C, L, step, W, N, 2, sc_multitaper_fft_f64_supported=1)
    assert lib.names(*queries) == ["sc_taper_windows_f64", "sc_fft_execute_f64"] and mem.plans == [(N, W * 65536 * K * C, True)]
    assert sp.R == 65536 and sp.strides == (W * 65536 * K * C, 65536 * K * C, K * C, C)
    lib, mem, sp = run(_stage_abc.spectra_f64, x64, h64, T, R, C, L, step, W, N, 2, sc_multitaper_fft_f64_supported=0)
    assert lib.names(*queries) == ["sc_taper_windows_f64", "sc_fft_execute_f64"] and mem.plans == [(N, W * R * K * C, True)]


def test_stage_b_call_sequences(monkeypatch):
    """_stage_abc.accumulate against the recording library: the float64 call and its ``which``, the planes-format calls (folded with
    the workspace, unfolded with the part count the library reports), the one-pass complex64 kernels with their leftover, the
    per-plane kernels -- and which descriptor (pad channel counted or not) each call gets."""
    from spectral_connectivity_amd import _lib, _stage_abc
    F, W, R, K, C, Ca = 17, 3, 2, 2, 3, 4
    n_bins, fpb, n_obs = 5, 8, 4
    CSM, ABS, SQ, SIGN, UNIT = _lib.PLANE_CSM, _lib.PLANE_ABS_IM, _lib.PLANE_IM_SQ, _lib.PLANE_SIGN_IM, _lib.PLANE_UNIT
    strides = _stage_abc.dense_strides(W, R, K, Ca)
    padded, real = ("desc", Ca, F), ("desc", C, F)

    def layout(d, planes, a, b, c, e):
        a._obj.value, b._obj.value, c._obj.value, e._obj.value = n_bins, fpb, 1, n_obs
        return 0

    def run(sp, planes, **kw):
        answers = {k: kw.pop(k) for k in list(kw) if k.startswith("sc_")}
        lib, mem = _RecordingLibrary(sc_accum_layout=layout, **answers), _numpy_memory()
        monkeypatch.setattr(_lib, "_lib", lib)
        rec, got_obs = _stage_abc.accumulate(mem, sp, "trials_tapers", planes, **kw)
        assert got_obs == n_obs and lib.names()[0] == "sc_accum_layout" and lib.args("sc_accum_layout")[0][0] == real
        return lib, mem, rec

    mem = _numpy_memory()
    X64 = mem.spectra(np.zeros((F, W, R, K, C), np.complex128), (F, W, R, K, C), _stage_abc.dense_strides(W, R, K, C), 32, True)
    X32 = mem.spectra(np.zeros((F, W, R, K, Ca), np.complex64), (F, W, R, K, C), strides, 32, True, C_alloc=Ca)
    P32 = mem.spectra(None, (F, W, R, K, C), strides, 32, True, C_alloc=Ca, P=np.zeros(64, np.uint8), scale=np.zeros(2 * Ca, np.float32))
    # float64 engine: everything, or the families the caller has not filled in ``out`` already
    lib, _, rec = run(X64, CSM | ABS)
    assert lib.names() == ["sc_accum_layout", "sc_accumulate_f64"] and rec.shape == (n_bins, fpb) and rec.dtype == np.float64
    assert lib.args("sc_accumulate_f64")[0][1:4] == (real, CSM | ABS, CSM | ABS)
    out = np.zeros((n_bins, fpb))
    lib, _, rec = run(X64, CSM | ABS, which=ABS, out=out)
    assert rec is out and lib.args("sc_accumulate_f64")[0][1:5] == (real, CSM | ABS, ABS, out.ctypes.data)
    assert run(X64, CSM, which=0, out=out)[0].names() == ["sc_accum_layout"]
    # planes format, folded: the adapter's workspace, its pointer and size
    lib, mem, rec = run(P32, CSM | ABS, workspace_owner="owner", sc_fused2_supported=1, sc_fused_workspace_bytes=400)
    assert lib.names() == ["sc_accum_layout", "sc_fused2_supported", "sc_fused_workspace_bytes", "sc_fused2_csm_absim_f32"]
    call = lib.args("sc_fused2_csm_absim_f32")[0]
    assert call[1] == padded and call[3:7] == (CSM | ABS, rec.ctypes.data, mem.workspaces[0].ctypes.data, 400) and rec.dtype == np.float32
    # planes format, unfolded: room for 1 + 400 // 160 parts, two of them used
    def two_parts(*args):
        args[7]._obj.value = 2
        return 0
    lib, mem, rec = run(P32, CSM | ABS, fold=False, sc_fused2_supported=1, sc_fused_workspace_bytes=400, sc_fused2_csm_absim_parts_f32=two_parts)
    assert lib.names()[-1] == "sc_fused2_csm_absim_parts_f32" and not mem.workspaces and rec.shape == (2, n_bins, fpb)
    call = lib.args("sc_fused2_csm_absim_parts_f32")[0]
    assert call[1] == padded and call[4] == rec.ctypes.data and call[5] == rec.ctypes.data + n_bins * fpb * 4 and call[6] == 2 * n_bins * fpb * 4
    assert run(P32, CSM | ABS, fold=False, sc_fused2_supported=1, sc_fused_workspace_bytes=100)[0].names()[-1] == "sc_fused2_csm_absim_f32"
    # one-pass complex64 kernels: what they cover on the padded descriptor, the leftover family on the real one
    every = CSM | ABS | SIGN | UNIT | SQ
    lib, mem, rec = run(X32, every, sc_fused_supported=1, sc_fused_planes_covered=every & ~SQ, sc_fused_workspace_bytes=64)
    assert lib.names() == ["sc_accum_layout", "sc_fused_supported", "sc_fused_planes_covered", "sc_fused_workspace_bytes",
                           "sc_fused_csm_absim_ws_f32", "sc_fused_sign_ws_f32", "sc_fused_unit_scratch_bytes", "sc_fused_unit_ws_f32",
                           "sc_nonlinear_accumulate_f32"]
    for name in ("sc_fused_csm_absim_ws_f32", "sc_fused_sign_ws_f32", "sc_fused_unit_ws_f32"):
        assert lib.args(name)[0][1:6] == (padded, every, rec.ctypes.data, mem.workspaces[0].ctypes.data, 64), name
    assert lib.args("sc_fused_unit_ws_f32")[0][6:8] == (None, 0) and lib.args("sc_fused_supported") == [(Ca,)]
    assert lib.args("sc_nonlinear_accumulate_f32")[0][1:4] == (real, every, SQ)
    # every plane through its own kernel on request: no unit-phasor MFMA pass
    lib, _, _ = run(X32, every, use_fused=False)
    assert lib.names() == ["sc_accum_layout", "sc_csm_accumulate_f32", "sc_nonlinear_accumulate_f32"]
    assert lib.args("sc_csm_accumulate_f32")[0][1] == real and lib.args("sc_nonlinear_accumulate_f32")[0][1:4] == (real, every, every & ~CSM)
    # a channel count the one-pass kernels do not take: CSM and the unit phasors on the f32 matrix cores, the rest on the VALU
    lib, _, _ = run(X32, every, sc_fused_supported=0, sc_unit_scratch_bytes=48)
    assert lib.names() == ["sc_accum_layout", "sc_fused_supported", "sc_csm_accumulate_f32", "sc_unit_scratch_bytes", "sc_unit_accumulate_f32",
                           "sc_nonlinear_accumulate_f32"]
    assert lib.args("sc_unit_accumulate_f32")[0][1] == real and lib.args("sc_unit_accumulate_f32")[0][5] == 48
    assert lib.args("sc_nonlinear_accumulate_f32")[0][1:4] == (real, every, every & ~CSM & ~UNIT)


def test_amplitude_guard_call_sequences(monkeypatch):
    """_stage_abc.amplitude_guard against the recording library: which requests are measured at all, the thresholds at the amplitudes
    of real recordings, the verdict per request from one measurement, the complex128 copy and the float64 record stage B then
    writes, the planes format's own criterion on its channel scales, and a group's decision handed in."""
    import ctypes

    from spectral_connectivity_amd import _lib, _stage_abc
    F, W, R, K, C, Ca = 17, 3, 2, 2, 3, 4
    n_bins, fpb, n_obs = 5, 8, 4
    CSM, ABS, SQ, SIGN, UNIT = _lib.PLANE_CSM, _lib.PLANE_ABS_IM, _lib.PLANE_IM_SQ, _lib.PLANE_SIGN_IM, _lib.PLANE_UNIT
    cross, every = CSM | ABS | SQ, CSM | ABS | SQ | SIGN | UNIT
    strides = _stage_abc.dense_strides(W, R, K, Ca)
    scan = ["sc_amplitude_range_work_bytes", "sc_amplitude_range_f32"]

    def layout(d, planes, a, b, c, e):
        a._obj.value, b._obj.value, c._obj.value, e._obj.value = n_bins, fpb, 1, n_obs
        return 0

    def amplitude(typical):
        """sc_amplitude_range_f32 reporting coefficients of root mean square ``typical`` and maximum 4 x that on every channel."""
        def fill(d_X, n_rows, n_ch, d_out, d_work, work_bytes, stream):
            out = np.ctypeslib.as_array(ctypes.cast(d_out, ctypes.POINTER(ctypes.c_double)), (2, n_ch))
            out[0], out[1] = typical ** 2 * n_rows, 4 * typical
            return 0
        return fill

    def memory():
        mem = _numpy_memory()
        mem.download = lambda a: a
        mem.read_scales = lambda sp: sp.scale
        return mem

    def guard(sp, planes, typical=1.0, decided=None, **answers):
        lib, mem = _RecordingLibrary(sc_accum_layout=layout, sc_amplitude_range_f32=amplitude(typical), **answers), memory()
        monkeypatch.setattr(_lib, "_lib", lib)
        return lib, mem, _stage_abc.amplitude_guard(mem, sp, planes, decided)

    def fresh():
        return memory().spectra(np.zeros((F, W, R, K, Ca), np.complex64), (F, W, R, K, C), strides, 32, True, C_alloc=Ca)

    # families that square no product, and complex128 spectra: nothing is measured
    sp = fresh()
    lib, _, got = guard(sp, CSM | ABS | SIGN)
    assert got is sp and not lib.names()
    X64 = memory().spectra(np.zeros((F, W, R, K, C), np.complex128), (F, W, R, K, C), _stage_abc.dense_strides(W, R, K, C), 32, True)
    lib, _, got = guard(X64, every)
    assert got is X64 and not lib.names()
    # measured once, over every row, with the workspace the query names
    lib, _, got = guard(sp, every, sc_amplitude_range_work_bytes=96)
    assert got is sp and lib.names() == scan and lib.args(scan[0]) == [(F * W * R * K, Ca)]
    assert lib.args(scan[1])[0][1:3] == (F * W * R * K, Ca) and lib.args(scan[1])[0][5] == 96
    assert not guard(sp, every)[0].names()                                  # (kept on the spectra object)
    # 2^-47 (MEG in tesla) is inside the float32 range for s / |s| and outside it for (Im s)^2; 2^-54 and 2^40 are outside for both
    # or one of them; volts (2^-24) and 24-bit counts (2^19) are inside for everything
    for typical, planes, wide in ((2.0 ** -47, UNIT, False), (2.0 ** -47, cross, True), (2.0 ** -54, UNIT, True), (2.0 ** 40, UNIT, False),
                                  (2.0 ** 40, cross, True), (2.0 ** -24, every, False), (2.0 ** 19, every, False)):
        sp = fresh()
        lib, mem, got = guard(sp, planes, typical)
        assert (got is not sp) == wide and got.f64 == wide, (typical, planes)
        assert lib.names() == scan + (["sc_spectra_widen_f32"] if wide else []), (typical, planes)
        if wide:
            assert lib.args("sc_spectra_widen_f32")[0][1] == F * W * R * K * Ca and got.X.dtype == np.complex128
            assert (got.F, got.W, got.R, got.K, got.C, got.C_alloc, got.strides) == (F, W, R, K, C, Ca, strides)
            rec, _ = _stage_abc.accumulate(mem, got, "trials_tapers", planes)         # the float64 engine's call, a float64 record
            assert lib.names()[-2:] == ["sc_accum_layout", "sc_accumulate_f64"] and rec.dtype == np.float64
    # the verdict is per request, the measurement and the copy per object: (Im s)^2 at 2^-47 is widened, s / |s| afterwards is not
    sp = fresh()
    _, _, wide1 = guard(sp, cross, 2.0 ** -47)
    lib, _, got = guard(sp, UNIT, 2.0 ** -47)
    assert wide1 is not sp and got is sp and not lib.names()
    lib, _, got = guard(sp, cross, 2.0 ** -47)
    assert got is wide1 and not lib.names()
    # a group's decision: no measurement here, the copy on True
    sp = fresh()
    lib, _, got = guard(sp, cross, decided=False)
    assert got is sp and not lib.names()
    lib, _, got = guard(sp, cross, decided=True)
    assert got.f64 and lib.names() == ["sc_spectra_widen_f32"]
    # planes-format spectra: the criterion is on the channel scales themselves (1 / scale 2^-30: volts; 2^-53: tesla), without a pass
    # over the data; a family the format does not serve (s / |s|) is measured on the decoded coefficients
    def planes_spectra(inverse):
        scale = np.concatenate([np.full(Ca, 1.0 / inverse, np.float32), np.full(Ca, inverse, np.float32)])
        return memory().spectra(None, (F, W, R, K, C), strides, 32, True, C_alloc=Ca, P=np.zeros(64, np.uint8), scale=scale)
    sp = planes_spectra(2.0 ** -30)
    lib, _, got = guard(sp, cross)
    assert got is sp and not lib.names()
    sp = planes_spectra(2.0 ** 13)                                           # (24-bit counts)
    assert guard(sp, cross)[2] is sp
    sp = planes_spectra(2.0 ** -53)
    lib, _, got = guard(sp, cross)
    assert got.f64 and lib.names() == ["sc_spectra_from_planes_f32", "sc_spectra_widen_f32"]


def test_tiled_record_refuses_a_block_of_another_type(monkeypatch):
    """engine._accumulate_blocked (more than 256 signals) places float32 tiles into a float32 record and float64 into float64: a block
    pair that came back as the other type is an error, never a silent cast (the sum of (Im s)^2 of tesla-scaled data would be 0)."""
    import torch

    from spectral_connectivity_amd import _lib, engine

    class Wide:
        C, f64, device = 300, False, torch.device("cpu")

    monkeypatch.setattr(engine, "accum_layout", lambda sp, et, planes, n_freq: (2, 4 * 190 * 256, 1, 6))      # 19 blocks of 16: 190 tiles
    monkeypatch.setattr(engine, "_channel_subset", lambda sp, cols: type("Sub", (), {"C": int(len(cols))})())
    seen = []

    def accumulate(sub, et, planes, n_freq=None, mark=None, guard=True):
        seen.append(guard)
        nb = -(-sub.C // 16)
        return torch.zeros((2, 4 * (nb * (nb + 1) // 2) * 256), dtype=torch.float64), 6

    monkeypatch.setattr(engine, "accumulate", accumulate)
    with pytest.raises(_lib.HipEngineError, match="float64"):
        engine._accumulate_blocked(Wide(), "trials_tapers", _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ, None, None, 1)
    assert seen == [False]                                                   # (the decision was the whole array's, taken before the tiling)


def test_stage_c_call_sequences(monkeypatch):
    """_stage_abc.measure / measure_multi against the recording library: shape and dtype of every kind of output, narrow and wide,
    the forms that sum partial records while they read, and the one-launch epilogue falling back to single calls."""
    from spectral_connectivity_amd import _lib, _stage_abc
    n_bins, fpb, C, n_obs = 5, 8, 3, 4
    lib, mem = _RecordingLibrary(), _numpy_memory()
    monkeypatch.setattr(_lib, "_lib", lib)
    rec = np.zeros((n_bins, fpb), np.float32)
    for which, tail, kinds in ((_lib.M_POWER, (C,), (np.float32, np.float64)), (_lib.M_COHERENCY, (C, C), (np.complex64, np.complex128)),
                               (_lib.M_WPLI, (C, C), (np.float32, np.float64))):
        for wide in (False, True):
            out = _stage_abc.measure(mem, rec, C, _lib.PLANE_CSM, n_obs, which, wide)
            assert out.shape == (n_bins,) + tail and out.dtype == kinds[wide]
            name, args = lib.calls[-1]
            assert name == ("sc_measure_f64" if wide else "sc_measure_f32")
            assert args[:7] == (rec.ctypes.data, n_bins, C, _lib.PLANE_CSM, n_obs, which, out.ctypes.data)
    assert _stage_abc.measure(mem, np.zeros((n_bins, fpb)), C, _lib.PLANE_CSM, n_obs, _lib.M_POWER, True) is not None
    assert lib.calls[-1][1][3] == _lib.PLANE_CSM | _lib.RECORD_F64
    parts = np.zeros((3, n_bins, fpb), np.float32)
    out = _stage_abc.measure(mem, parts[0], C, _lib.PLANE_CSM, n_obs, _lib.M_COHERENCY, True, parts=parts)
    name, args = lib.calls[-1]
    assert name == "sc_measure_parts" and out.dtype == np.complex128
    assert args[:11] == (parts.ctypes.data, parts[1].ctypes.data, 3, n_bins * fpb, n_bins, C, _lib.PLANE_CSM, n_obs, _lib.M_COHERENCY,
                         out.ctypes.data, 1)
    # several measures: one launch for two to four real-valued C x C ones, single calls otherwise
    two = [_lib.M_COHERENCE_MAGNITUDE, _lib.M_WPLI]
    del lib.calls[:]
    outs = _stage_abc.measure_multi(mem, rec, C, _lib.PLANE_CSM, n_obs, two, False)
    assert lib.names() == ["sc_measure_multi_f32"] and [o.shape for o in outs] == [(n_bins, C, C)] * 2 and outs[0].dtype == np.float32
    args = lib.calls[-1][1]
    assert args[:6] == (rec.ctypes.data, n_bins, C, _lib.PLANE_CSM, n_obs, 2) and list(args[6]) == two
    assert [args[7][k] for k in range(2)] == [o.ctypes.data for o in outs]
    del lib.calls[:]
    outs = _stage_abc.measure_multi(mem, parts[0], C, _lib.PLANE_CSM, n_obs, two[:1], True, parts=parts)
    assert lib.names() == ["sc_measure_multi_parts"] and outs[0].dtype == np.float64
    assert lib.calls[-1][1][:4] == (parts.ctypes.data, parts[1].ctypes.data, 3, n_bins * fpb) and lib.calls[-1][1][8] == 1
    for which in (two[:1], two + [_lib.M_PLV, _lib.M_PLI, _lib.M_PPC], two + [_lib.M_COHERENCY]):
        del lib.calls[:]
        outs = _stage_abc.measure_multi(mem, rec, C, _lib.PLANE_CSM, n_obs, which, True)
        assert lib.names() == ["sc_measure_f64"] * len(which) and [a[5] for a in lib.args("sc_measure_f64")] == which
        assert [o.dtype for o in outs] == [np.complex128 if w == _lib.M_COHERENCY else np.float64 for w in which]
