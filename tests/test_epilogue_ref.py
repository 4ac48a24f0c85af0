"""CPU-only checks of the epilogue reference (tests/epilogue_ref.py) that tests/test_gpu_epilogue.py compares the device with:
its extended-precision measures against the nine oracle functions on sums of random coefficients, its record packer against
conftest.unpack_record_planes, and its layout numbers against include/sc_hip.h and hand-counted tiles."""
import os
import re

import numpy as np
import pytest

import epilogue_ref as eref
from conftest import ROOT, unpack_record_planes
from oracle import spectral_oracle as so

PLANE_SETS = (eref.PLANE_CSM, eref.PLANE_UNIT, eref.PLANE_SIGN_IM, eref.PLANE_CSM | eref.PLANE_ABS_IM,
              eref.PLANE_CSM | eref.PLANE_ABS_IM | eref.PLANE_IM_SQ,
              eref.PLANE_CSM | eref.PLANE_ABS_IM | eref.PLANE_IM_SQ | eref.PLANE_SIGN_IM, eref.PLANES_ALL)


def random_sums(rng, n_bins, C):
    """Full-matrix sums with the symmetries of real ones and a different number in every slot (the Im-derived diagonals too,
    which the measures must ignore)."""
    a = rng.standard_normal((n_bins, C, C)) + 1j * rng.standard_normal((n_bins, C, C))
    u = rng.standard_normal((n_bins, C, C)) + 1j * rng.standard_normal((n_bins, C, C))
    sym = rng.random((3, n_bins, C, C))
    up = np.triu(np.ones((C, C), dtype=bool), 1)

    def herm(z):
        z = np.where(up, z, 0)
        return z + z.conj().swapaxes(-1, -2)

    s, unit = herm(a), herm(u)
    d = np.arange(C)
    s[:, d, d] = C + rng.random((n_bins, C))
    unit[:, d, d] = rng.random((n_bins, C))
    ab, sq, sg = (np.where(up, x, 0) for x in sym)
    return {"s": s, "unit": unit, "abs_im": ab + ab.swapaxes(-1, -2) + np.eye(C) * 0.3, "im_sq": sq + sq.swapaxes(-1, -2) + np.eye(C) * 0.7,
            "sign_im": sg - sg.swapaxes(-1, -2) + np.eye(C) * 0.5}


def test_measures_ref_against_the_oracle():
    """2 windows x 5 trials x 3 tapers x 8 bins x 7 channels, "trials_tapers": identical NaN patterns, within 16 eps cond."""
    rng = np.random.default_rng(5)
    W, R, K, N, C = 2, 5, 3, 8, 7
    coef = rng.standard_normal((W, R, K, N, C)) + 1j * rng.standard_normal((W, R, K, N, C))
    F = N // 2 + 1
    # the oracle's own float64 sums (its mean is this sum / n), so that the comparison is of the formulas, not of two summations
    sums = {k: v[:, :F].reshape(W * F, C, C) for k, v in eref.sums_from_coefficients(coef, axes=(1, 2)).items()}
    val, cond = eref.measures_ref(sums, R * K)
    assert set(eref.REAL_MEASURES) <= set(val) and set(cond) == set(eref.REAL_MEASURES)
    worst = {}
    for name in eref.REAL_MEASURES:
        want = so.MEASURES[name](coef).reshape(W * F, C, C)
        worst[name] = eref.worst_ratio(want, val[name], cond[name])
        off = ~np.eye(C, dtype=bool)
        assert np.isfinite(want[:, off]).all(), name
    print("\n  oracle against measures_ref, |diff| / (eps cond): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= 16.0, worst
    # power and the complex-valued ones, at the same bound with |value| as the scale
    p = so.power(coef).reshape(W * F, C)
    assert np.abs(p - val["power"]).max() <= 16 * eref.EPS * np.abs(p).max()
    cy = so.coherency(coef).reshape(W * F, C, C)
    got = val["coherency"][..., 0] + 1j * val["coherency"][..., 1]
    assert np.array_equal(np.isnan(cy), np.isnan(got.astype(np.complex128)))
    assert np.nanmax(np.abs(cy - got)) <= 16 * eref.EPS
    plv = so._plv_complex(coef, "trials_tapers").reshape(W * F, C, C)
    assert np.abs(plv - (val["plv_complex"][..., 0] + 1j * val["plv_complex"][..., 1])).max() <= 16 * eref.EPS


def test_measures_ref_does_not_mirror():
    """The lower triangle comes from the sums of the lower triangle: spoiling one entry (j, i) changes that entry alone."""
    sums = random_sums(np.random.default_rng(2), 2, 5)
    base, _ = eref.measures_ref(sums, 12)
    for key in sums:
        sums[key] = sums[key].copy()
        sums[key][1, 3, 1] = 100.0
    spoiled, _ = eref.measures_ref(sums, 12)
    for name in eref.REAL_MEASURES:
        diff = np.argwhere(np.nan_to_num(base[name].astype(np.float64), nan=-7) != np.nan_to_num(spoiled[name].astype(np.float64), nan=-7))
        assert diff.tolist() == [[1, 3, 1]], (name, diff.tolist())


@pytest.mark.parametrize("C", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("planes", PLANE_SETS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_record_round_trip(C, planes, dtype):
    sums = random_sums(np.random.default_rng(C), 3, C)
    for k in sums:                                       # float32-representable, so both record types hold the same numbers
        sums[k] = sums[k].astype(np.complex64 if np.iscomplexobj(sums[k]) else np.float32)
    lay = eref.layout(C, planes)
    rec = eref.pack_record(sums, C, planes, dtype, fill=-77.0)
    assert rec.dtype == dtype and rec.shape == (3, lay.floats_per_bin)
    back = unpack_record_planes(rec, C)                  # [3, n_planes, C, C]
    stack = eref.plane_stack(sums, planes)
    assert back.shape == stack.shape
    upper = np.triu(np.ones((C, C), dtype=bool))
    assert np.array_equal(back[:, :, upper], stack[:, :, upper])
    # below the diagonal: the fill inside diagonal tiles, nothing stored elsewhere
    lower = ~upper
    same_tile = (np.arange(C)[:, None] // 16) == (np.arange(C)[None, :] // 16)
    assert (back[:, :, lower & same_tile] == -77.0).all() and np.isnan(back[:, :, lower & ~same_tile]).all()
    # every element of the record is an upper entry or the fill: pad rows and columns included
    n_upper = C * (C + 1) // 2
    assert int((rec != -77.0).sum()) == 3 * lay.n_planes * n_upper
    nan_rec = eref.pack_record(sums, C, planes, dtype, fill=np.nan)
    assert int(np.isnan(nan_rec).sum()) == int((rec == -77.0).sum())


def test_layout_numbers():
    """The plane masks and measure numbers of include/sc_hip.h; tile counts and indices counted by hand."""
    with open(os.path.join(ROOT, "include", "sc_hip.h")) as f:
        header = f.read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SC_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", header)}
    assert (defs["SC_PLANE_CSM"], defs["SC_PLANE_ABS_IM"], defs["SC_PLANE_IM_SQ"], defs["SC_PLANE_SIGN_IM"], defs["SC_PLANE_UNIT"]) == (
        eref.PLANE_CSM, eref.PLANE_ABS_IM, eref.PLANE_IM_SQ, eref.PLANE_SIGN_IM, eref.PLANE_UNIT)
    header_ids = {"power": "POWER", "csm": "CSM", "coherency": "COHERENCY", "coherence_magnitude": "COHERENCE_MAGNITUDE",
                  "coherence_phase": "COHERENCE_PHASE", "imaginary_coherence": "IMAGINARY_COHERENCE", "phase_locking_value": "PLV",
                  "phase_lag_index": "PLI", "weighted_phase_lag_index": "WPLI", "debiased_squared_phase_lag_index": "DEBIASED_PLI2",
                  "debiased_squared_weighted_phase_lag_index": "DEBIASED_WPLI2", "pairwise_phase_consistency": "PPC",
                  "plv_complex": "PLV_COMPLEX"}
    assert {k: defs["SC_M_" + v] for k, v in header_ids.items()} == eref.MEASURE_IDS
    assert "tile index = bi*NB - bi*(bi-1)/2 + (bj-bi)" in header                    # the formula layout() restates
    from spectral_connectivity_amd import _lib                                       # (imports without a GPU: nothing is loaded)
    assert {k: _lib.MEASURE_PLANES[v] for k, v in eref.MEASURE_IDS.items()} == eref.MEASURE_PLANES
    for C, NB, n_tiles in ((1, 1, 1), (16, 1, 1), (17, 2, 3), (33, 3, 6), (100, 7, 28), (256, 16, 136), (260, 17, 153)):
        lay = eref.layout(C, eref.PLANES_ALL)
        assert (lay.NB, lay.n_tiles, lay.n_planes, lay.floats_per_bin) == (NB, n_tiles, 7, 7 * n_tiles * 256)
        # row-major over the upper triangle: consecutive, none twice
        idx = [lay.tile_index(bi, bj) for bi in range(NB) for bj in range(bi, NB)]
        assert idx == list(range(n_tiles))
    assert eref.layout(33, eref.PLANES_ALL).offset == {0x01: 0, 0x02: 2, 0x04: 3, 0x08: 4, 0x10: 5}
    assert eref.layout(33, eref.PLANE_UNIT).offset == {0x10: 0} and eref.layout(33, eref.PLANE_UNIT).n_planes == 2
    assert eref.layout(33, eref.PLANE_CSM | eref.PLANE_SIGN_IM | eref.PLANE_UNIT).offset == {0x01: 0, 0x08: 2, 0x10: 3}
