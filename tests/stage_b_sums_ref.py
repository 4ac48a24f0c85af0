"""The yardstick of the float64 stage B (csrc/sc_f64.hip): the un-normalised sums a record holds, in numpy.longdouble, the
magnitude sums their rounding bounds are made of, the bounds, and a float64 restatement of the device arithmetic summed in
another order (what the bounds are checked against on the CPU, tests/test_stage_b_sums_ref.py).  NumPy only.

Conventions: s = x_i conj x_j per observation, so Re s = ar_i ar_j + ai_i ai_j and d = Im s = ai_i ar_j - ar_i ai_j; entry
[i, j] of every matrix is the pair (i, j).  The matrices here are FULL C x C; the checks (worst_ratios) read the upper triangle
i <= j, diagonal included -- the half every consumer of a record reads (the epilogue mirrors it; csrc/sc_measure.hip).

Bounds, u = 2^-53, n observations per bin, |err| of an entry of the un-normalised record:
    Re S, Im S      (2 n + 18) u T         T_re = sum |ar_i ar_j| + |ai_i ai_j|, T_im = sum M, M = |ai_i ar_j| + |ar_i ai_j|:
                                           2 n fused multiply-adds in any order, up to 16 parts added by the combine kernel
    sum |d|         (n + 26) u sum M       a computed d is off by at most 2 u M, contracted or not; n - 1 additions of
                                           non-negative terms; the combine additions
    sum d^2         (n + 26) u sum M^2     (d + e)^2 with |e| <= 2 u M <= d^2 + 4 u M^2 (+ its own rounding), then as above
    sum sign(d)     0                      provided no observation has |d| <= 4 u M (near_zero == 0): twice the error of a
                                           computed d, so its sign is the sign of the exact one
    sum s / |s|     (2 n + 50) u T_unit    T of the unit phasors x / |x|: a phasor component from a correctly rounded sqrt and
                                           division (x^2 + y^2: 2 u, sqrt halves it and rounds: 2 u, 1 / : 3 u, the product: 4 u)
                                           gives 8 u per product, 32 u over the four of a pair, on top of the 2 n + 18
The longdouble sums themselves are off by at most 2 n 2^-64 T: a 2048th of the smallest bound.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).eps > 2.0 ** -63:
    import pytest
    pytest.skip(f"numpy.longdouble has eps {float(np.finfo(LD).eps):.3g} here, not the 2^-63 of an extended-precision type: no "
                "reference more precise than the float64 kernels under test", allow_module_level=True)

U = 2.0 ** -53
PLANES = ("S_re", "S_im", "A", "Q", "G", "U_re", "U_im")          # record order: CSM (2), |Im s|, (Im s)^2, sign, unit (2)
FAMILY_PLANES = {0x01: ("S_re", "S_im"), 0x02: ("A",), 0x04: ("Q",), 0x08: ("G",), 0x10: ("U_re", "U_im")}
SLAB = 32                                                          # observations per slab of the per-observation temporaries


def record_plane_names(planes):
    """Names (PLANES) of the planes of a record of the families ``planes``, in record order."""
    return [name for bit in (0x01, 0x02, 0x04, 0x08, 0x10) if planes & bit for name in FAMILY_PLANES[bit]]


def coefficients(F, n_obs, C, seed):
    """The data recipe of the float32 launch-plan sweep (tests/test_gpu_planes.py), complex128 [F, n_obs, C]: complex normal
    coefficients, a shared component (0.4 x channel 0, before the scales: no cancelling pairs), channel scales over six decades."""
    rng = np.random.default_rng(seed)
    coef = rng.standard_normal((F, n_obs, C)) + 1j * rng.standard_normal((F, n_obs, C))
    coef = coef + 0.4 * coef[..., :1]
    return coef * (0.2 + rng.random(C)) * 10.0 ** rng.integers(-3, 4, C)


def stage_b_sums(coef, slab=SLAB):
    """complex128 coefficients [F, n_obs, C] of ONE group -> dict of longdouble arrays [F, C, C] -- S_re, S_im, A = sum |d|,
    Q = sum d^2, G = sum sign(d), U_re, U_im = sum x_i conj x_j / (|x_i| |x_j|) (0 / 0 = NaN, like the reference's s / |s|) -- the
    magnitude sums T_re, T_im (= sum M), M2 (= sum M^2), TU_re, TU_im of the bounds, and ``near_zero``: the number of
    (observation, pair i < j) with |d| <= 4 u M.  One bin and at most ``slab`` <= 128 observations at a time."""
    coef = np.asarray(coef)
    assert coef.dtype == np.complex128 and coef.ndim == 3 and 1 <= slab <= 128
    F, n_obs, C = coef.shape
    names = PLANES + ("T_re", "T_im", "M2", "TU_re", "TU_im")
    out = {k: np.zeros((F, C, C), dtype=LD) for k in names}
    strict = np.triu(np.ones((C, C), dtype=bool), 1)
    near_zero = 0
    for f in range(F):
        for o0 in range(0, n_obs, slab):
            x = coef[f, o0:o0 + slab]
            ar, ai = x.real.astype(LD), x.imag.astype(LD)
            aar, aai = np.abs(ar), np.abs(ai)
            # what is bilinear in the two channels: sums over the slab as matrix products
            out["S_re"][f] += ar.T @ ar + ai.T @ ai
            out["S_im"][f] += ai.T @ ar - ar.T @ ai
            out["T_re"][f] += aar.T @ aar + aai.T @ aai
            out["T_im"][f] += aai.T @ aar + aar.T @ aai
            p = aar * aai
            out["M2"][f] += (ai * ai).T @ (ar * ar) + (ar * ar).T @ (ai * ai) + 2 * (p.T @ p)
            with np.errstate(invalid="ignore", divide="ignore"):
                mag = np.sqrt(ar * ar + ai * ai)
                ur, ui = ar / mag, ai / mag
            out["U_re"][f] += ur.T @ ur + ui.T @ ui
            out["U_im"][f] += ui.T @ ur - ur.T @ ui
            aur, aui = np.abs(ur), np.abs(ui)
            out["TU_re"][f] += aur.T @ aur + aui.T @ aui
            out["TU_im"][f] += aui.T @ aur + aur.T @ aui
            # per observation: d and M, [slab, C, C]
            d = ai[:, :, None] * ar[:, None, :] - ar[:, :, None] * ai[:, None, :]
            M = aai[:, :, None] * aar[:, None, :] + aar[:, :, None] * aai[:, None, :]
            ad = np.abs(d)
            near_zero += int(np.count_nonzero((ad <= 4 * U * M)[:, strict]))
            del M
            out["A"][f] += ad.sum(axis=0)
            out["G"][f] += np.sign(d).sum(axis=0)
            out["Q"][f] += (d * d).sum(axis=0)
            del d, ad
    out["near_zero"] = near_zero
    out["n_obs"] = n_obs
    return out


def bounds(sums):
    """{plane: [F, C, C] longdouble bound on |err|} from stage_b_sums (module docstring)."""
    n = sums["n_obs"]
    return {"S_re": (2 * n + 18) * U * sums["T_re"], "S_im": (2 * n + 18) * U * sums["T_im"],
            "A": (n + 26) * U * sums["T_im"], "Q": (n + 26) * U * sums["M2"], "G": np.zeros_like(sums["G"]),
            "U_re": (2 * n + 50) * U * sums["TU_re"], "U_im": (2 * n + 50) * U * sums["TU_im"]}


def _ratio(err, bound):
    """err / bound; where the bound is 0 (a sign sum, a zero channel): 0 for no error, inf for any."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)


def worst_ratios(got, names, sums, against=None, factor=1):
    """Worst |got - ref| / (factor x bound) per plane over the UPPER triangle (i <= j, the diagonal included) of the planes
    ``got`` [F, len(names), C, C] (float64; the lower triangle is never read).  ``against`` [F, len(names), C, C]: compare with
    these values instead of the reference sums (two device results, factor = 2).  Entries whose reference is NaN (unit phasors of
    a zero channel) must be NaN in ``got`` too and are left out; returns {plane: ratio}, inf for a NaN that should not be one."""
    b = bounds(sums)
    C = got.shape[-1]
    upper = np.triu(np.ones((C, C), dtype=bool))
    worst = {}
    for k, name in enumerate(names):
        g = got[:, k][:, upper].astype(LD)
        ref = (sums[name] if against is None else against[:, k].astype(LD))[:, upper]
        bound = factor * b[name][:, upper]
        nan_ref = np.isnan(sums[name][:, upper])
        if not np.array_equal(np.isnan(g), nan_ref) or (against is not None and not np.array_equal(np.isnan(ref), nan_ref)):
            worst[name] = np.inf
            continue
        ok = ~nan_ref
        worst[name] = float(_ratio(np.abs(g[ok] - ref[ok]), bound[ok]).max()) if ok.any() else 0.0
    return worst


def restatement_f64(coef, chunk=16):
    """The device arithmetic restated in float64 NumPy, summed in ANOTHER order than any kernel's (observations from the last to
    the first, partial sums per ``chunk`` of them added at the end): [F, 7, C, C] float64 in PLANES order, full matrices."""
    coef = np.asarray(coef, dtype=np.complex128)[:, ::-1]
    F, n_obs, C = coef.shape
    parts = []
    for o0 in range(0, n_obs, chunk):
        x = coef[:, o0:o0 + chunk]
        ar, ai = x.real, x.imag
        d = ai[:, :, :, None] * ar[:, :, None, :] - ar[:, :, :, None] * ai[:, :, None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            un = x / np.abs(x)
        ur, ui = un.real, un.imag
        t = lambda a: np.swapaxes(a, 1, 2)
        parts.append(np.stack([t(ar) @ ar + t(ai) @ ai, t(ai) @ ar - t(ar) @ ai, np.abs(d).sum(1), (d * d).sum(1), np.sign(d).sum(1),
                               t(ur) @ ur + t(ui) @ ui, t(ui) @ ur - t(ur) @ ui], axis=1))
    rec = parts[-1]
    for p in parts[-2::-1]:
        rec = rec + p
    return rec


def grouped_observations(coef5, axes):
    """Spectra [F, W, R, K, C] reduced over ``axes`` (indices into (window, trial, taper): EXPECTATION_AXES) -> [n_groups * F,
    n_obs, C], bins in the order of a record (group-major, groups in (window, trial, taper) order of the kept axes)."""
    F, C = coef5.shape[0], coef5.shape[-1]
    kept = [a for a in range(3) if a not in axes]
    x = np.transpose(coef5, [1 + a for a in kept] + [0] + [1 + a for a in axes] + [4])
    n_obs = int(np.prod([coef5.shape[1 + a] for a in axes]))
    return np.ascontiguousarray(x.reshape(-1, n_obs, C)), n_obs
