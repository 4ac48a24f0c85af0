"""NumPy float64 reference of partial and multiple coherence, in two forms that share no step.

S [..., C, C]: Hermitian cross-spectral matrices, S_ij = E[x_i conj(x_j)].  Both forms return (partial coherency complex128
[..., C, C] with a NaN diagonal, multiple coherence magnitude float64 [..., C]):

    inverse    G = S^-1: -G_ij / sqrt(G_ii G_jj) and sqrt(max(0, 1 - 1 / (S_ii G_ii)))
    residual   per pair p = (i, j) with r the other channels, the Schur complement S_pp - S_pr S_rr^-1 S_rp -- the cross-spectrum
               of what is left of the pair after regressing it on r -- then the ordinary coherency of that 2 x 2 block; per
               channel i, 1 - (S_ii - S_ir S_rr^-1 S_ri) / S_ii, the explained share of its power
"""
import numpy as np


def inverse(S):
    S = np.asarray(S, dtype=complex)
    C = S.shape[-1]
    G = np.linalg.inv(S)
    g = np.einsum("...ii->...i", G).real
    gamma = -G / np.sqrt(g[..., :, None] * g[..., None, :])
    gamma[..., np.arange(C), np.arange(C)] = np.nan
    s = np.einsum("...ii->...i", S).real
    return gamma, np.sqrt(np.maximum(0.0, 1.0 - 1.0 / (s * g)))


def _schur(S, p, r):
    """S_pp - S_pr S_rr^-1 S_rp (S_pp itself when r is empty)."""
    Spp = S[..., p, :][..., :, p]
    if not r:
        return Spp
    Spr, Srr = S[..., p, :][..., :, r], S[..., r, :][..., :, r]
    return Spp - Spr @ np.linalg.solve(Srr, np.conj(np.swapaxes(Spr, -1, -2)))


def residual(S):
    S = np.asarray(S, dtype=complex)
    C = S.shape[-1]
    gamma = np.full(S.shape, np.nan, dtype=complex)
    multiple = np.empty(S.shape[:-1])
    for i in range(C):
        for j in range(i + 1, C):
            E = _schur(S, [i, j], [k for k in range(C) if k not in (i, j)])
            c = E[..., 0, 1] / np.sqrt(E[..., 0, 0].real * E[..., 1, 1].real)
            gamma[..., i, j], gamma[..., j, i] = c, np.conj(c)
        e = _schur(S, [i], [k for k in range(C) if k != i])[..., 0, 0].real
        multiple[..., i] = np.sqrt(np.maximum(0.0, 1.0 - e / S[..., i, i].real))
    return gamma, multiple


def coherency(S):
    """The ordinary coherency S_ij / sqrt(S_ii S_jj), NaN diagonal."""
    S = np.asarray(S, dtype=complex)
    C = S.shape[-1]
    s = np.einsum("...ii->...i", S).real
    out = S / np.sqrt(s[..., :, None] * s[..., None, :])
    out[..., np.arange(C), np.arange(C)] = np.nan
    return out


def common_driver_spectrum(n_fft=32, tau=(3, 5), noise=(0.3, 0.4)):
    """Two-sided spectrum [n_fft, 3, 3] of x1 = z(t - tau1) + n1, x2 = z(t - tau2) + n2, x3 = z with z an AR(1) process and white
    n1, n2: S(f) = sigma(f) a a^H + diag(s1, s2, 0), a = (e^{-i w tau1}, e^{-i w tau2}, 1).  x1 and x2 are coherent only through z,
    so their partial coherence is zero while their coherence is sigma / sqrt((sigma + s1)(sigma + s2)); the others explain the
    share sigma q / (1 + sigma q), q = 1 / s1 + 1 / s2, of the power of x3 (the residual form with Sherman-Morrison).  Returns
    (S, sigma [n_fft], (s1, s2))."""
    w = 2 * np.pi * np.arange(n_fft) / n_fft
    sigma = 1.0 / np.abs(1.0 - 0.3 * np.exp(-1j * w)) ** 2
    a = np.stack([np.exp(-1j * w * tau[0]), np.exp(-1j * w * tau[1]), np.ones(n_fft)], axis=-1)
    S = sigma[:, None, None] * a[:, :, None] * np.conj(a[:, None, :])
    S = S + np.diag([noise[0], noise[1], 0.0])[None]
    return S, sigma, noise
