"""CPU checks of the NumPy reference of MIC / MIM (tests/imaginary_interaction_ref.py): its three forms agree, and it has the
properties of Ewald et al. 2012 that the device tests rely on."""
import numpy as np

import imaginary_interaction_ref as iref


def random_csm(C, n_bins, seed, n_obs=None):
    """[n_bins, C, C] normalised cross-spectral matrices X X^H / n of correlated complex observations."""
    rng = np.random.default_rng(seed)
    n_obs = n_obs or 2 * C + 3
    X = rng.standard_normal((n_bins, C, n_obs)) + 1j * rng.standard_normal((n_bins, C, n_obs))
    mix = np.eye(C) + 0.4 * (rng.standard_normal((C, C)) + 0.5j * rng.standard_normal((C, C)))
    X = mix @ X
    return X @ np.conj(np.swapaxes(X, -1, -2)) / n_obs


def block_mix(C, groups, rng, complex_=False):
    T = np.zeros((C, C), dtype=complex if complex_ else float)
    for g in groups:
        k = len(g)
        B = np.eye(k) + 0.6 * rng.standard_normal((k, k))
        if complex_:
            B = B + 0.6j * rng.standard_normal((k, k))
        T[np.ix_(g, g)] = B
    return T


def test_three_forms_agree():
    S = random_csm(9, 6, 1)
    a, b = np.array([0, 4, 7]), np.array([1, 2, 5, 8])
    mic_e, mim_e = iref.interaction_ewald(S, a, b)
    mic_c, mim_c = iref.interaction_cholesky(S, a, b)
    mim_t = iref.interaction_trace(S, a, b)
    assert mic_e.shape == (6,) and np.all(mic_e > 0.05)
    np.testing.assert_allclose(mic_c, mic_e, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(mim_c, mim_e, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(mim_t, mim_e, rtol=1e-12, atol=1e-12)
    labels = np.array([0, 1, 1, 2, 0, 1, 2, 0, 1])
    e = iref.interaction(S, labels)
    c = iref.interaction(S, labels, form="cholesky")
    for x, y in zip(e[:2], c[:2]):
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.isnan(x[:, [0, 1, 2], [0, 1, 2]]).all()
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(x, np.swapaxes(x, -1, -2))


def test_single_channels_are_imaginary_coherence():
    S = random_csm(4, 5, 2)
    for i, j in ((0, 1), (2, 3), (3, 0)):
        mic, mim = iref.interaction_ewald(S, [i], [j])
        icoh = np.abs(S[:, i, j].imag) / np.sqrt(S[:, i, i].real * S[:, j, j].real)
        np.testing.assert_allclose(mic, icoh, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(mim, icoh ** 2, rtol=1e-12, atol=1e-14)


def test_real_mixing_inside_groups_leaves_both_unchanged():
    rng = np.random.default_rng(3)
    S = random_csm(7, 4, 3)
    groups = [np.array([0, 2, 3]), np.array([1, 4, 5, 6])]
    T = block_mix(7, groups, rng)
    mixed = T @ S @ T.T
    for got, want in zip(iref.interaction_ewald(mixed, *groups), iref.interaction_ewald(S, *groups)):
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10)


def test_complex_mixing_changes_mic():
    rng = np.random.default_rng(4)
    S = random_csm(6, 4, 4)
    groups = [np.array([0, 1, 2]), np.array([3, 4, 5])]
    T = block_mix(6, groups, rng, complex_=True)
    mixed = T @ S @ np.conj(T.T)
    assert np.abs(iref.interaction_ewald(mixed, *groups)[0] - iref.interaction_ewald(S, *groups)[0]).max() > 1e-3


def test_real_cross_spectrum_gives_zero():
    S = random_csm(6, 3, 5).real + 0j
    for form in (iref.interaction_ewald, iref.interaction_cholesky):
        mic, mim = form(S, [0, 1], [2, 3, 4, 5])
        assert np.all(mic == 0.0) and np.all(mim == 0.0)
    assert np.all(iref.interaction_trace(S, [0, 1], [2, 3, 4, 5]) == 0.0)


def test_bounds():
    for seed, (na, nb) in enumerate([(1, 1), (1, 5), (3, 3), (4, 7), (6, 2)]):
        S = random_csm(na + nb, 8, 10 + seed, n_obs=na + nb + 1)
        mic, mim = iref.interaction_ewald(S, np.arange(na), na + np.arange(nb))
        k = min(na, nb)
        assert np.all(mic >= 0.0) and np.all(mic <= 1.0 + 1e-12)
        assert np.all(mic ** 2 <= mim * (1 + 1e-12)) and np.all(mim <= k * mic ** 2 * (1 + 1e-12)) and np.all(mim <= k + 1e-12)
