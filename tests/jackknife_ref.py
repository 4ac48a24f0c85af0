"""NumPy float64 reference of the delete-one jackknife of power and coherence (Thomson & Chave 1991; Chronux coherencyc /
mtspectrumc with err = [2 p]), the yardstick of Connectivity.jackknife.

For one kept index and bin the delete units u = 1 .. n hold g observations each; G_u = sum over the unit's observations of
x_i conj(x_j), S = sum_u G_u.  With d_u = theta(S without u) - theta(S) and m = mean_u d_u:

    estimate = theta(S),  bias_corrected = theta(S) - (n - 1) m,  standard_error = sqrt((n - 1) / n sum_u (d_u - m)^2)

    "power"                theta = ln(S_ii / n_observations_used)          (n g for the full estimate, (n - 1) g without a unit)
    "coherence_magnitude"  theta = arctanh(|S_ij| / sqrt(S_ii S_jj))       diagonal NaN
    "imaginary_coherence"  theta = Im(S_ij) / sqrt(S_ii S_jj), signed      diagonal NaN
    "linear_power"         theta = S_ii / n_observations_used              (untransformed; for the exact identity only)

Two forms that must agree: ``jackknife`` subtracts G_u from S; ``jackknife_brute_force`` deletes the unit from the coefficient
array and recomputes from scratch.  Coefficients: (n_time_windows, n_trials, n_tapers, n_fft_samples, n_signals); outputs on the
non-negative frequencies, kept axes first.  A channel without power in a bin is NaN in its entries; a coherence magnitude that
rounds to 1 or more gives arctanh's inf / NaN as NumPy returns them.
"""
import numpy as np

EXPECTATION_AXES = {"time": (0,), "trials": (1,), "tapers": (2,), "time_trials": (0, 1), "time_tapers": (0, 2),
                    "trials_tapers": (1, 2), "time_trials_tapers": (0, 1, 2)}
MEASURES = ("power", "coherence_magnitude", "imaginary_coherence", "linear_power")


def units(coefficients, expectation_type, over):
    """[kept..., n units, g observations, n_freq, C] complex128 view of the non-negative bins."""
    x = np.asarray(coefficients, dtype=np.complex128)
    x = x[:, :, :, :x.shape[3] // 2 + 1]
    axes = EXPECTATION_AXES[expectation_type]
    kept = [a for a in (0, 1, 2) if a not in axes]
    if over == "trials":
        if 1 not in axes:
            raise ValueError("over='trials' needs an expectation over trials")
        inside = [a for a in axes if a != 1]
        x = np.transpose(x, kept + [1] + inside + [3, 4])
        shape = x.shape
        n_kept = len(kept)
        g = int(np.prod(shape[n_kept + 1:n_kept + 1 + len(inside)], dtype=int))
        x = x.reshape(shape[:n_kept] + (shape[n_kept], g) + shape[-2:])
    elif over == "observations":
        x = np.transpose(x, kept + list(axes) + [3, 4])
        n_kept = len(kept)
        n = int(np.prod(x.shape[n_kept:n_kept + len(axes)], dtype=int))
        x = x.reshape(x.shape[:n_kept] + (n, 1) + x.shape[-2:])
    else:
        raise ValueError("over must be 'trials' or 'observations'")
    if x.shape[-4] < 2:
        raise ValueError("a jackknife needs at least two units")
    return x


def _csm(x):
    """sum over the unit and observation axes (-4, -3) of x_i conj(x_j): [..., n_freq, C, C]"""
    return np.einsum("...ugfi,...ugfj->...fij", x, np.conj(x))


def _theta(S, n_obs_used, measure):
    p = np.real(np.einsum("...ii->...i", S))
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "linear_power":
            return p / n_obs_used
        if measure == "power":
            return np.where(p > 0, np.log(np.where(p > 0, p, 1.0) / n_obs_used), np.nan)
        norm = np.sqrt(p[..., :, None] * p[..., None, :])
        if measure == "coherence_magnitude":
            out = np.arctanh(np.abs(S) / norm)
        elif measure == "imaginary_coherence":
            out = np.imag(S) / norm
        else:
            raise ValueError(measure)
    C = S.shape[-1]
    out[..., np.arange(C), np.arange(C)] = np.nan
    return out


def _finish(theta, d):
    """d: [n units, ...] deviations from theta"""
    n = d.shape[0]
    m = d.mean(axis=0)
    return dict(estimate=theta, bias_corrected=theta - (n - 1) * m,
                standard_error=np.sqrt((n - 1) / n * ((d - m) ** 2).sum(axis=0)))


def jackknife(coefficients, expectation_type="trials_tapers", measures=("coherence_magnitude",), over="trials"):
    """Subtract form: S - G_u.  Returns {measure: {estimate, bias_corrected, standard_error}}."""
    x = units(coefficients, expectation_type, over)
    n, g = x.shape[-4], x.shape[-3]
    S = _csm(x)
    out = {}
    for measure in measures:
        theta = _theta(S, n * g, measure)
        d = np.empty((n,) + theta.shape)
        for u in range(n):
            G = _csm(x[..., u:u + 1, :, :, :])
            d[u] = _theta(S - G, (n - 1) * g, measure) - theta
        out[measure] = _finish(theta, d)
    return out


def jackknife_brute_force(coefficients, expectation_type="trials_tapers", measures=("coherence_magnitude",), over="trials"):
    """The unit is deleted from the coefficient array and everything is recomputed from scratch."""
    x = units(coefficients, expectation_type, over)
    n, g = x.shape[-4], x.shape[-3]
    out = {}
    for measure in measures:
        theta = _theta(_csm(x), n * g, measure)
        d = np.empty((n,) + theta.shape)
        for u in range(n):
            d[u] = _theta(_csm(np.delete(x, u, axis=-4)), (n - 1) * g, measure) - theta
        out[measure] = _finish(theta, d)
    return out


def mixed_noise(W, R, K, F, C, seed=0, mix=0.4):
    """Complex Gaussian noise mixed by I + mix N(0, 1): coefficients (W, R, K, N = 2 F - 2, C) whose non-negative bins are the F
    independent draws (the bins beyond are their conjugate mirrors, which no jackknife reads)."""
    rng = np.random.default_rng(seed)
    M = np.eye(C) + mix * rng.standard_normal((C, C))
    z = (rng.standard_normal((W, R, K, F, C)) + 1j * rng.standard_normal((W, R, K, F, C))) / np.sqrt(2.0)
    half = z @ M.T
    N = 2 * F - 2
    out = np.empty((W, R, K, N, C), dtype=np.complex128)
    out[..., :F, :] = half
    out[..., F:, :] = np.conj(half[..., N - F:0:-1, :])
    return out
