"""float64 NumPy reference of seed-based connectivity (csrc/sc_seed.hip): the sums the accumulate kernel forms, from the
coefficients -- per (seed, target) and bin, over the averaged axes, with s = x_seed conj(x_target) --, and the formulas the seed
epilogue applies to them (csrc/sc_measure_value.h).  Nothing here calls the package or the oracle: tests/test_seed_connectivity_ref.py
holds it to the oracle's ten functions, the GPU tests use both."""
import numpy as np

EPS = np.finfo(np.float64).eps
EXPECTATION_AXES = {"time": (0,), "trials": (1,), "tapers": (2,), "time_trials": (0, 1), "time_tapers": (0, 2),
                    "trials_tapers": (1, 2), "time_trials_tapers": (0, 1, 2)}
MEASURES = ("coherency", "coherence_magnitude", "coherence_phase", "imaginary_coherence", "phase_locking_value",
            "pairwise_phase_consistency", "phase_lag_index", "weighted_phase_lag_index", "debiased_squared_phase_lag_index",
            "debiased_squared_weighted_phase_lag_index")


def seed_sums(coef, seeds, targets, expectation_type="trials_tapers"):
    """The un-normalised sums of a seed record on the non-negative bins, each [kept axes..., n_freq, n_seeds, n_targets] (the
    powers [..., n_seeds] and [..., n_targets]), and n_observations.  ``coef``: [W, R, K, N, C] complex."""
    coef = np.asarray(coef, dtype=np.complex128)
    axes = EXPECTATION_AXES[expectation_type]
    n_freq = coef.shape[3] // 2 + 1
    x = coef[:, :, :, :n_freq]
    xs, xt = x[..., np.asarray(seeds)], x[..., np.asarray(targets)]
    s = xs[..., :, None] * np.conj(xt[..., None, :])
    diag = np.asarray(seeds)[:, None] == np.asarray(targets)[None, :]
    im = np.where(diag, 0.0, s.imag)                                    # Im forced to 0 where a seed is its own target
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = s / np.abs(s)                                            # 0 / 0 = NaN, like the reference's s / abs(s)
    total = lambda a: a.sum(axis=axes)
    sums = dict(s=total(s.real) + 1j * total(im), abs_im=total(np.abs(im)), im_sq=total(im ** 2), sign_im=total(np.sign(im)),
                unit=total(unit), power_seed=total(np.abs(xs) ** 2), power_target=total(np.abs(xt) ** 2), diag=diag)
    return sums, int(np.prod([coef.shape[a] for a in axes]))


def seed_measures(sums, n, measures=MEASURES):
    """{name: values} from the sums of ``seed_sums`` and the observation count ``n``: the reference's formulas
    (connectivity.py:632-1159) entry for entry, the diagonal rules where a seed is its own target."""
    diag = sums["diag"]
    s = sums["s"] / n
    norm = np.maximum(np.sqrt((sums["power_seed"] / n)[..., :, None] * (sums["power_target"] / n)[..., None, :]), EPS)
    coherency = np.where(diag, np.nan, s / norm)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for name in measures:
            if name == "coherency":
                out[name] = coherency
            elif name == "coherence_magnitude":
                out[name] = np.clip(np.abs(coherency) ** 2, 0, 1)
            elif name == "coherence_phase":
                out[name] = np.angle(coherency)
            elif name == "imaginary_coherence":
                out[name] = np.clip(np.abs(s.imag / norm), 0, 1)
            elif name == "phase_locking_value":
                out[name] = np.abs(sums["unit"] / n)
            elif name == "pairwise_phase_consistency":
                out[name] = ((sums["unit"] * np.conj(sums["unit"]) - n) / (n ** 2 - n)).real
            elif name == "phase_lag_index":
                out[name] = sums["sign_im"] / n
            elif name == "debiased_squared_phase_lag_index":
                out[name] = (n * (sums["sign_im"] / n) ** 2 - 1.0) / (n - 1.0)
            elif name == "weighted_phase_lag_index":
                w = sums["abs_im"] / n
                out[name] = s.imag / np.where(w < EPS, 1.0, w)
            elif name == "debiased_squared_weighted_phase_lag_index":
                w = sums["abs_im"] ** 2 - sums["im_sq"]
                out[name] = (sums["s"].imag ** 2 - sums["im_sq"]) / np.where(w == 0, np.nan, w)
            else:
                raise KeyError(name)
    return out


def seed_connectivity(coef, seeds, targets=None, measures=MEASURES, expectation_type="trials_tapers"):
    targets = np.arange(np.asarray(coef).shape[-1]) if targets is None else targets
    sums, n = seed_sums(coef, seeds, targets, expectation_type)
    return seed_measures(sums, n, measures)


def from_full(full, seeds, targets):
    """[..., seeds, :][..., targets] of an all-pairs array."""
    return np.asarray(full)[..., np.asarray(seeds), :][..., np.asarray(targets)]
