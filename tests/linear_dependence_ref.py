"""NumPy float64 reference of Pascual-Marqui's total, instantaneous and lagged linear dependence between two groups of signals
(Pascual-Marqui 2007, arXiv:0706.1776; Pascual-Marqui et al. 2011, Phil. Trans. R. Soc. A 369:3768).

S: [..., C, C] Hermitian normalised cross-spectral matrices (one per kept-axes group and bin); a, b: the signal indices of two
disjoint groups, J = a then b.
    F_total         = ln det S_aa    + ln det S_bb    - ln det S_JJ
    F_instantaneous = ln det Re S_aa + ln det Re S_bb - ln det Re S_JJ
    F_lagged        = F_total - F_instantaneous
in two forms that share no step:
  logdet     slogdet of the three blocks, as defined;
  canonical  Cholesky whitening of the two group blocks, the SVD of the whitened cross block, -sum log1p(-sigma^2) -- once on S and
             once on Re S;
and, for two single signals with coherency c, the closed forms
    F_total = -ln(1 - |c|^2),  F_inst = -ln(1 - (Re c)^2),  F_lagged = ln(1 + (Im c)^2 / (1 - |c|^2)),
    lagged coherence rho^2_lag = 1 - exp(-F_lagged) = (Im c)^2 / (1 - (Re c)^2).
"""
import numpy as np


def var_spectrum(C, seed, n_fft=32):
    """The well-conditioned VAR(1) spectra of the MIC tests (test_gpu_imaginary_interaction.var_spectrum)."""
    from test_gpu_imaginary_interaction import var_spectrum as mic_var_spectrum
    return mic_var_spectrum(C, seed, n_fft)


def _herm(x):
    return np.conj(np.swapaxes(x, -1, -2))


def _block(S, r, c):
    return S[..., np.asarray(r)[:, None], np.asarray(c)[None, :]]


def _logdet(M):
    sign, ld = np.linalg.slogdet(M)
    return np.where(np.real(sign) > 0, ld, np.nan)


def _dependence_logdet(S, a, b):
    J = np.concatenate([a, b])
    return _logdet(_block(S, a, a)) + _logdet(_block(S, b, b)) - _logdet(_block(S, J, J))


def dependence_logdet(S, a, b):
    """(total, instantaneous, lagged) by the log-determinants of the blocks."""
    S = np.asarray(S, dtype=complex)
    a, b = np.asarray(a), np.asarray(b)
    total, inst = _dependence_logdet(S, a, b), _dependence_logdet(S.real, a, b)
    return total, inst, total - inst


def _canonical_sigma(S, a, b):
    """Singular values of L_a^-1 S_ab L_b^-H with S_gg = L_g L_g^H: the canonical coherences (magnitudes) of the pair."""
    La, Lb = np.linalg.cholesky(_block(S, a, a)), np.linalg.cholesky(_block(S, b, b))
    M = np.linalg.solve(La, _block(S, a, b))
    M = _herm(np.linalg.solve(Lb, _herm(M)))
    return np.linalg.svd(M, compute_uv=False)


def dependence_canonical(S, a, b):
    """(total, instantaneous, lagged) as -sum log1p(-sigma^2) over the canonical coherences of S and of Re S."""
    S = np.asarray(S, dtype=complex)
    a, b = np.asarray(a), np.asarray(b)
    total = -np.log1p(-_canonical_sigma(S, a, b) ** 2).sum(axis=-1)
    inst = -np.log1p(-_canonical_sigma(S.real, a, b) ** 2).sum(axis=-1)
    return total, inst, total - inst


def canonical_coherences_squared(S, a, b):
    """rho_k^2 as the eigenvalues of S_aa^-1 S_ab S_bb^-1 S_ba by two linear solves (no factorisation, no SVD)."""
    S = np.asarray(S, dtype=complex)
    a, b = np.asarray(a), np.asarray(b)
    X = np.linalg.solve(_block(S, a, a), _block(S, a, b))
    Y = np.linalg.solve(_block(S, b, b), _block(S, b, a))
    return np.sort(np.linalg.eigvals(X @ Y).real, axis=-1)


def coherency(S, i, j):
    S = np.asarray(S, dtype=complex)
    return S[..., i, j] / np.sqrt(S[..., i, i].real * S[..., j, j].real)


def dependence_closed(c):
    """(total, instantaneous, lagged) of two single signals with coherency c."""
    c = np.asarray(c, dtype=complex)
    m2 = np.abs(c) ** 2
    return -np.log(1 - m2), -np.log(1 - c.real ** 2), np.log(1 + c.imag ** 2 / (1 - m2))


def lagged_coherence_closed(c):
    c = np.asarray(c, dtype=complex)
    return c.imag ** 2 / (1 - c.real ** 2)


def dependence(S, group_labels=None, form="logdet"):
    """(total, instantaneous, lagged [..., G, G], labels) for every pair of the groups np.unique(group_labels) (None: every signal
    its own group); symmetric, NaN diagonal."""
    S = np.asarray(S)
    C = S.shape[-1]
    group_labels = np.arange(C) if group_labels is None else np.asarray(group_labels)
    labels = np.unique(group_labels)
    groups = [np.flatnonzero(group_labels == lab) for lab in labels]
    G = len(labels)
    out = [np.full(S.shape[:-2] + (G, G), np.nan) for _ in range(3)]
    fn = dependence_canonical if form == "canonical" else dependence_logdet
    for i in range(G):
        for j in range(i + 1, G):
            for o, v in zip(out, fn(S, groups[i], groups[j])):
                o[..., i, j] = o[..., j, i] = v
    return out[0], out[1], out[2], labels


def pairwise_closed(S):
    """(total, instantaneous, lagged, lagged coherence) [..., C, C] of every pair of single signals by the closed forms."""
    S = np.asarray(S, dtype=complex)
    d = np.sqrt(np.einsum("...ii->...i", S).real)
    c = S / (d[..., :, None] * d[..., None, :])
    eye = np.eye(S.shape[-1], dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = [np.where(eye, np.nan, v) for v in dependence_closed(c) + (lagged_coherence_closed(c),)]
    return tuple(res)
