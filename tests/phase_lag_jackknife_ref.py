"""NumPy float64 reference of the delete-one jackknife of the phase-lag family (the jackknife of FieldTrip's ft_connectivity_wpli),
the yardstick of Connectivity.jackknife for "phase_lag_index", "weighted_phase_lag_index", "debiased_squared_phase_lag_index" and
"debiased_squared_weighted_phase_lag_index".

For one kept index, bin and channel pair (i, j), s = x_i conj(x_j) of one observation; the delete units u = 1 .. n hold g
observations each (jackknife_ref.units).  Over a set of m observations A = sum Im s, B = sum |Im s|, N = sum sign(Im s)
(sign(0) = 0), Q = sum (Im s)^2 and

    phase_lag_index                             theta = N / m                                            antisymmetric
    weighted_phase_lag_index                    theta = (A / m) / w, w = B / m, w = 1 where w < 2^-52    antisymmetric
    debiased_squared_phase_lag_index            theta = (m (N / m)^2 - 1) / (m - 1)                      symmetric
    debiased_squared_weighted_phase_lag_index   theta = (A^2 - Q) / (B^2 - Q), NaN where B^2 - Q == 0    symmetric

all on the identity scale, diagonal NaN.  The full estimate takes all m = n g observations, a delete-one value the m = (n - 1) g
others; d_u = theta(without u) - theta(all), mean = mean_u d_u:

    estimate = theta(all),  bias_corrected = theta(all) - (n - 1) mean,  standard_error = sqrt((n - 1) / n sum_u (d_u - mean)^2)

Two forms that must agree: ``jackknife`` subtracts the unit's sums from the totals; ``jackknife_brute_force`` deletes the unit from
the coefficient array and sums again from scratch.
"""
import numpy as np

from jackknife_ref import units

MEASURES = ("phase_lag_index", "weighted_phase_lag_index", "debiased_squared_phase_lag_index",
            "debiased_squared_weighted_phase_lag_index")
ANTISYMMETRIC = ("phase_lag_index", "weighted_phase_lag_index")
EPS = 2.0 ** -52


def _im(x):
    """Im(x_i conj(x_j)) of every observation: [..., units, g, n_freq, C, C]"""
    return x.imag[..., :, None] * x.real[..., None, :] - x.real[..., :, None] * x.imag[..., None, :]


def _sums(im):
    """(A, B, N, Q) over the unit and observation axes (-5, -4) of im"""
    axes = (-5, -4)
    return im.sum(axes), np.abs(im).sum(axes), np.sign(im).sum(axes), (im * im).sum(axes)


def _theta(A, B, N, Q, m, measure):
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "phase_lag_index":
            out = N / m
        elif measure == "debiased_squared_phase_lag_index":
            out = (m * (N / m) ** 2 - 1.0) / (m - 1.0)
        elif measure == "weighted_phase_lag_index":
            w = B / m
            w = np.where(w < EPS, 1.0, w)
            out = (A / m) / w
        elif measure == "debiased_squared_weighted_phase_lag_index":
            den = B * B - Q
            out = (A * A - Q) / np.where(den == 0, np.nan, den)
        else:
            raise ValueError(measure)
    out = np.array(out, dtype=np.float64)
    C = out.shape[-1]
    out[..., np.arange(C), np.arange(C)] = np.nan
    return out


def _finish(theta, d):
    n = d.shape[0]
    m = d.mean(axis=0)
    return dict(estimate=theta, bias_corrected=theta - (n - 1) * m,
                standard_error=np.sqrt((n - 1) / n * ((d - m) ** 2).sum(axis=0)))


def jackknife(coefficients, expectation_type="trials_tapers", measures=MEASURES, over="trials"):
    """Subtract form.  Returns {measure: {estimate, bias_corrected, standard_error}}."""
    x = units(coefficients, expectation_type, over)
    n, g = x.shape[-4], x.shape[-3]
    im = _im(x)
    total = _sums(im)
    per_unit = [_sums(im[..., u:u + 1, :, :, :, :]) for u in range(n)]
    out = {}
    for measure in measures:
        theta = _theta(*total, n * g, measure)
        d = np.empty((n,) + theta.shape)
        for u in range(n):
            d[u] = _theta(*(t - s for t, s in zip(total, per_unit[u])), (n - 1) * g, measure) - theta
        out[measure] = _finish(theta, d)
    return out


def jackknife_brute_force(coefficients, expectation_type="trials_tapers", measures=MEASURES, over="trials"):
    """The unit is deleted from the coefficient array and everything is summed again from scratch."""
    x = units(coefficients, expectation_type, over)
    n, g = x.shape[-4], x.shape[-3]
    out = {}
    for measure in measures:
        theta = _theta(*_sums(_im(x)), n * g, measure)
        d = np.empty((n,) + theta.shape)
        for u in range(n):
            d[u] = _theta(*_sums(_im(np.delete(x, u, axis=-4))), (n - 1) * g, measure) - theta
        out[measure] = _finish(theta, d)
    return out


def _two_sided(half):
    """(W, R, K, F, C) non-negative bins -> (W, R, K, N = 2 F - 2, C) coefficients (the bins beyond are conjugate mirrors, which
    no jackknife reads)."""
    F = half.shape[3]
    N = 2 * F - 2
    out = np.empty(half.shape[:3] + (N, half.shape[4]), dtype=np.complex128)
    out[..., :F, :] = half
    out[..., F:, :] = np.conj(half[..., N - F:0:-1, :])
    return out


def lagged_noise(W, R, K, F, C, seed=0, mix=0.4):
    """Complex Gaussian noise mixed by the COMPLEX matrix I + mix (N + i N): the channels lead and lag each other, so the true
    wPLI is not 0 (a real mixing matrix, jackknife_ref.mixed_noise, gives a real cross-spectrum and wPLI around 0 only)."""
    rng = np.random.default_rng(seed)
    M = np.eye(C) + mix * (rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
    z = (rng.standard_normal((W, R, K, F, C)) + 1j * rng.standard_normal((W, R, K, F, C))) / np.sqrt(2.0)
    return _two_sided(z @ M.T)


def margin_phases(W, R, K, F, C, seed=0):
    """Coefficients r e^{i phi} whose every product x_i conj(x_j), i != j, keeps a margin from the real axis: per observation the
    channels sit in distinct slots k pi / (C + 1), k = 1 .. C (a random permutation), plus a random offset in {0, pi}, a jitter
    of at most pi / (8 (C + 1)), one common random phase and a random amplitude in [0.5, 2].  Two phases then differ by
    (k - k') pi / (C + 1) + {0, pi} + at most pi / (4 (C + 1)), so |sin| of the difference is at least sin(3 pi / (4 (C + 1)))
    -- asserted below; >= 0.069 for C <= 33, where no float32 rounding (2^-24 per product) flips a sign."""
    rng = np.random.default_rng(seed)
    shape = (W, R, K, F, C)
    slots = rng.permuted(np.broadcast_to(np.arange(1, C + 1), shape), axis=-1)
    phi = slots * np.pi / (C + 1) + np.pi * rng.integers(0, 2, shape)
    phi = phi + rng.uniform(-1.0, 1.0, shape) * np.pi / (8 * (C + 1)) + rng.uniform(0, 2 * np.pi, shape[:4] + (1,))
    half = rng.uniform(0.5, 2.0, shape) * np.exp(1j * phi)
    s = half[..., :, None] * np.conj(half[..., None, :])
    rel = np.abs(s.imag) / (np.abs(half)[..., :, None] * np.abs(half)[..., None, :])
    off = ~np.eye(C, dtype=bool)
    margin = np.sin(3 * np.pi / (4 * (C + 1)))
    assert rel[..., off].min() >= margin * (1 - 1e-12), (rel[..., off].min(), margin)
    return _two_sided(half)
