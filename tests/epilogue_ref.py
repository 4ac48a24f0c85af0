"""Reference for the measures epilogue (csrc/sc_measure.hip) on records built by hand: the record layout restated, a packer
that is the inverse of conftest.unpack_record_planes, and the measures in extended precision.  NumPy only.

A set of sums is a dict of [n_bins, C, C] arrays over the FULL matrix (both triangles, as the sums over observations of the
per-observation cross products s = x_i conj(x_j) would be):
    "s"        complex   sum s                (Hermitian; the diagonal holds the powers)
    "abs_im"   real      sum |Im s|           (symmetric)
    "im_sq"    real      sum (Im s)^2         (symmetric)
    "sign_im"  real      sum sign Im s        (antisymmetric)
    "unit"     complex   sum s / |s|          (Hermitian)
pack_record places the entries with i <= j only -- what the epilogue is documented to read -- and ``fill`` everywhere else.
measures_ref evaluates entry (i, j) from the sums at (i, j), the lower triangle as well: it never mirrors a result.
"""
from types import SimpleNamespace

import numpy as np

# include/sc_hip.h: SC_PLANE_*, SC_M_* (tests/test_epilogue_ref.py reads the header and compares)
PLANE_CSM, PLANE_ABS_IM, PLANE_IM_SQ, PLANE_SIGN_IM, PLANE_UNIT = 0x01, 0x02, 0x04, 0x08, 0x10
PLANES_ALL = 0x1F
TILE, TILE_ELEMS = 16, 256
MEASURE_IDS = {"power": 0, "csm": 1, "coherency": 2, "coherence_magnitude": 3, "coherence_phase": 4, "imaginary_coherence": 5,
               "phase_locking_value": 6, "phase_lag_index": 7, "weighted_phase_lag_index": 8, "debiased_squared_phase_lag_index": 9,
               "debiased_squared_weighted_phase_lag_index": 10, "pairwise_phase_consistency": 11, "plv_complex": 12}
REAL_MEASURES = ("coherence_magnitude", "coherence_phase", "imaginary_coherence", "phase_locking_value", "phase_lag_index",
                 "weighted_phase_lag_index", "debiased_squared_phase_lag_index", "debiased_squared_weighted_phase_lag_index",
                 "pairwise_phase_consistency")
MEASURE_PLANES = {"power": PLANE_CSM, "csm": PLANE_CSM, "coherency": PLANE_CSM, "coherence_magnitude": PLANE_CSM,
                  "coherence_phase": PLANE_CSM, "imaginary_coherence": PLANE_CSM, "phase_locking_value": PLANE_UNIT,
                  "plv_complex": PLANE_UNIT, "pairwise_phase_consistency": PLANE_UNIT, "phase_lag_index": PLANE_SIGN_IM,
                  "debiased_squared_phase_lag_index": PLANE_SIGN_IM, "weighted_phase_lag_index": PLANE_CSM | PLANE_ABS_IM,
                  "debiased_squared_weighted_phase_lag_index": PLANE_CSM | PLANE_ABS_IM | PLANE_IM_SQ}
# the planes of a bin record in storage order: (mask, number of planes, key of the sums, parts)
_PLANE_ORDER = ((PLANE_CSM, "s", ("real", "imag")), (PLANE_ABS_IM, "abs_im", (None,)), (PLANE_IM_SQ, "im_sq", (None,)),
                (PLANE_SIGN_IM, "sign_im", (None,)), (PLANE_UNIT, "unit", ("real", "imag")))
EPS = np.finfo(np.float64).eps


def layout(C, planes):
    """sc_n_blocks, sc_n_tiles, sc_tile_index, sc_plane_count and sc_plane_offset of csrc/sc_common.h for ``C`` signals and the
    plane mask ``planes``: NB, n_tiles, n_planes, offset {mask: first plane}, floats_per_bin, tile_index(bi, bj)."""
    NB = (C + TILE - 1) // TILE
    offset, n = {}, 0
    for mask, _, parts in _PLANE_ORDER:
        if planes & mask:
            offset[mask] = n
            n += len(parts)
    n_tiles = NB * (NB + 1) // 2
    return SimpleNamespace(C=C, NB=NB, n_tiles=n_tiles, n_planes=n, offset=offset, floats_per_bin=n * n_tiles * TILE_ELEMS,
                           tile_index=lambda bi, bj: bi * NB - bi * (bi - 1) // 2 + (bj - bi))


def complete(upper, sign):
    """The full matrices [..., C, C] whose entries i <= j are those of ``upper`` and whose entry (j, i) is sign x entry (i, j):
    +1 symmetric, -1 antisymmetric (the imaginary part of a Hermitian matrix; a zero becomes -0 below the diagonal, as a complex
    conjugate's does)."""
    upper = np.asarray(upper, dtype=np.float64)
    C = upper.shape[-1]
    return np.where(np.triu(np.ones((C, C), dtype=bool)), upper, sign * upper.swapaxes(-1, -2))


def as_complex(re, im):
    """re + i im without the products of a complex multiplication (0 x Inf = NaN)."""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def plane_stack(sums, planes):
    """[n_bins, n_planes, C, C] float64: the planes of ``planes`` in storage order."""
    out = []
    for mask, key, parts in _PLANE_ORDER:
        if planes & mask:
            out += [np.asarray(sums[key] if p is None else getattr(np.asarray(sums[key]), p), dtype=np.float64) for p in parts]
    return np.stack(out, axis=1)


def pack_record(sums, C, planes, dtype, fill=0.0):
    """The record [n_bins, floats_per_bin] of ``dtype`` holding the entries i <= j of the sums; ``fill`` in every element the
    epilogue must not use: the strict lower triangle inside diagonal tiles and every row or column >= C."""
    lay = layout(C, planes)
    stack = plane_stack(sums, planes)
    n_bins = stack.shape[0]
    P = lay.NB * TILE
    padded = np.full((n_bins, lay.n_planes, P, P), fill, dtype=np.float64)
    upper = np.triu(np.ones((C, C), dtype=bool))
    padded[:, :, :C, :C] = np.where(upper, stack, fill)
    rec = np.empty((n_bins, lay.n_planes, lay.n_tiles, TILE, TILE), dtype=np.float64)
    for bi in range(lay.NB):
        for bj in range(bi, lay.NB):
            rec[:, :, lay.tile_index(bi, bj)] = padded[:, :, bi * TILE:(bi + 1) * TILE, bj * TILE:(bj + 1) * TILE]
    with np.errstate(over="ignore"):
        return rec.reshape(n_bins, lay.floats_per_bin).astype(dtype)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def measures_ref(sums, n_obs):
    """(values, cond): every measure of the epilogue in np.longdouble (complex ones as (re, im) stacked on a last axis), and per
    real-valued measure the conditioning term the error of a float64 evaluation scales with.  The reference's formulas as
    oracle/spectral_oracle.py cites them: S / max(sqrt(P_i P_j), eps) with a NaN diagonal, clip to [0, 1], Im s forced to 0
    on the diagonal, wPLI weights < eps -> 1, debiased wPLI weight == 0 -> NaN.  Missing sums: the measures that need them
    are left out."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no extended precision here: no reference"
    n = np.longdouble(n_obs)
    val, cond = {}, {}
    with np.errstate(all="ignore"):
        d = np.arange(np.asarray(next(iter(sums.values()))).shape[-1])

        def zero_diag(a):
            a = _ld(a).copy()
            a[..., d, d] = 0
            return a

        if "s" in sums:
            s = np.asarray(sums["s"])
            s_re, s_im = _ld(s.real), zero_diag(s.imag)
            p = s_re[..., d, d] / n
            val["power"] = p
            val["csm"] = np.stack([s_re / n, s_im / n], axis=-1)
            den = np.maximum(np.sqrt(p[..., :, None] * p[..., None, :]), np.longdouble(EPS))
            c_re, c_im = s_re / n / den, s_im / n / den
            c_re[..., d, d] = np.nan
            c_im[..., d, d] = np.nan
            val["coherency"] = np.stack([c_re, c_im], axis=-1)
            val["coherence_magnitude"] = np.clip(c_re * c_re + c_im * c_im, 0, 1)
            val["coherence_phase"] = np.arctan2(c_im, c_re)
            val["imaginary_coherence"] = np.clip(np.abs(s_im / n / den), 0, 1)
            cond["coherence_magnitude"] = np.abs(val["coherence_magnitude"])
            cond["coherence_phase"] = np.ones_like(c_re)
            cond["imaginary_coherence"] = np.abs(val["imaginary_coherence"])
        if "unit" in sums:
            u = np.asarray(sums["unit"])
            u_re, u_im = _ld(u.real), _ld(u.imag)
            uu = u_re * u_re + u_im * u_im
            val["plv_complex"] = np.stack([u_re / n, u_im / n], axis=-1)
            val["phase_locking_value"] = np.hypot(u_re, u_im) / n
            val["pairwise_phase_consistency"] = (uu - n) / (n * n - n)
            cond["phase_locking_value"] = np.abs(val["phase_locking_value"])
            cond["pairwise_phase_consistency"] = (uu + n) / (n * n - n)
        if "sign_im" in sums:
            pli = zero_diag(sums["sign_im"]) / n
            val["phase_lag_index"] = pli
            val["debiased_squared_phase_lag_index"] = (n * pli * pli - 1) / (n - 1)
            cond["phase_lag_index"] = np.abs(pli)
            cond["debiased_squared_phase_lag_index"] = (n * pli * pli + 1) / (n - 1)
        if "s" in sums and "abs_im" in sums:
            sa = zero_diag(sums["abs_im"])
            w = sa / n
            w[w < EPS] = 1
            val["weighted_phase_lag_index"] = s_im / n / w
            cond["weighted_phase_lag_index"] = np.abs(val["weighted_phase_lag_index"])
            if "im_sq" in sums:
                sq = zero_diag(sums["im_sq"])
                wgt = sa * sa - sq
                wgt[wgt == 0] = np.nan
                q = (s_im * s_im - sq) / wgt
                val["debiased_squared_weighted_phase_lag_index"] = q
                cond["debiased_squared_weighted_phase_lag_index"] = ((s_im * s_im + sq) + np.abs(q) * (sa * sa + sq)) / np.abs(wgt)
    return val, cond


def worst_ratio(got, ref, cond):
    """max |got - ref| / (2^-52 cond) over the entries where the reference is finite (0 / 0 counts as 0: an exact entry under a zero
    bound), after checking that NaNs sit at the same places and infinities are equal.  ``got``: float64."""
    got, ref, cond = np.asarray(got, dtype=np.float64), np.asarray(ref), np.asarray(cond)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), f"NaN pattern differs at {np.argwhere(nan_g != nan_r)[:5].tolist()} (got NaN: {int(nan_g.sum())}, reference: {int(nan_r.sum())})"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf].astype(np.float64)), "infinite entries differ"
    fin = ~nan_r & ~inf
    assert np.isfinite(got[fin]).all(), "non-finite result where the reference is finite"
    with np.errstate(all="ignore"):
        err = np.abs(got[fin].astype(np.longdouble) - ref[fin])
        ratio = np.where(err == 0, 0, err / (np.longdouble(EPS) * cond[fin]))
    return float(ratio.max()) if ratio.size else 0.0


def sums_from_coefficients(coef, axes=(0,)):
    """The five sets of sums from complex coefficients [..., C], summed over ``axes``: per-observation outer products
    x conj(x)^T by np.matmul and the functions of them the reference averages (connectivity.py:447-492), in float64."""
    a = np.asarray(coef, dtype=np.complex128)[..., np.newaxis]
    s = np.matmul(a, a.swapaxes(-1, -2).conj())
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = (s / np.abs(s)).sum(axis=axes)
    return {"s": s.sum(axis=axes), "abs_im": np.abs(s.imag).sum(axis=axes), "im_sq": (s.imag ** 2).sum(axis=axes),
            "sign_im": np.sign(s.imag).sum(axis=axes), "unit": unit}
