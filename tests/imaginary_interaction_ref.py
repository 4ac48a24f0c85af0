"""NumPy float64 reference of the multivariate imaginary coherence between two groups of channels (Ewald, Marzetti, Zappasodi,
Meinecke & Nolte 2012, "Estimating true brain connectivity from EEG/MEG data invariant to linear and static transformations in
sensor space", NeuroImage 62:1964-1971): maximized imaginary coherence (MIC) and the multivariate interaction measure (MIM).

S: [..., C, C] Hermitian normalised cross-spectral matrices (one per kept-axes group and bin); a, b: the channel indices of two
disjoint groups.  R_a = Re S_aa, R_b = Re S_bb, I = Im S_ab, D = R_a^-1/2 I R_b^-1/2 with singular values sigma_1 >= sigma_2 ...:
    MIC = sigma_1,   MIM = sum_k sigma_k^2
in three forms that share no step:
  ewald     symmetric square-root whitening of the real group blocks (eigendecompositions), then the SVD of D;
  trace     MIM = tr(R_a^-1 I R_b^-1 I^T) by linear solves, no factorisation;
  cholesky  the device's form: S' has the group blocks R_a, R_b and the cross block i I; M = L_a^-1 (i I) L_b^-H with the Cholesky
            factors L_g of R_g, B = M M^H: MIC^2 = lambda_max(B), MIM = trace(B).
"""
import numpy as np


def _herm(x):
    return np.conj(np.swapaxes(x, -1, -2))


def _blocks(S, a, b):
    S = np.asarray(S, dtype=complex)
    a, b = np.asarray(a), np.asarray(b)
    return S[..., a[:, None], a[None, :]].real, S[..., b[:, None], b[None, :]].real, S[..., a[:, None], b[None, :]].imag


def _inv_sqrt(R):
    w, V = np.linalg.eigh(R)
    return (V * (1.0 / np.sqrt(w))[..., None, :]) @ np.swapaxes(V, -1, -2)


def interaction_ewald(S, a, b):
    """(MIC, MIM) by symmetric whitening and an SVD (Ewald et al. 2012, eqs. 8-14)."""
    Ra, Rb, I = _blocks(S, a, b)
    D = _inv_sqrt(Ra) @ I @ _inv_sqrt(Rb)
    sv = np.linalg.svd(D, compute_uv=False)
    return sv[..., 0], (sv ** 2).sum(axis=-1)


def interaction_trace(S, a, b):
    """MIM = tr(R_a^-1 I R_b^-1 I^T) by two linear solves."""
    Ra, Rb, I = _blocks(S, a, b)
    X = np.linalg.solve(Ra, I)                                       # R_a^-1 I
    Y = np.linalg.solve(Rb, np.swapaxes(I, -1, -2))                  # R_b^-1 I^T
    return np.einsum("...ij,...ji->...", X, Y)


def interaction_cholesky(S, a, b):
    """(MIC, MIM) from S' = [[R_a, i I], [-i I^T, R_b]] as canonical coherence reads S: Cholesky factors of the group blocks,
    M = L_a^-1 S'_ab L_b^-H, the largest eigenvalue and the trace of M M^H."""
    Ra, Rb, I = _blocks(S, a, b)
    La, Lb = np.linalg.cholesky(Ra + 0j), np.linalg.cholesky(Rb + 0j)
    M = np.linalg.solve(La, 1j * I)                                  # L_a^-1 (i I)
    M = _herm(np.linalg.solve(Lb, _herm(M)))                         # ... L_b^-H
    B = M @ _herm(M)
    lam = np.linalg.eigvalsh(B)[..., -1]
    return np.sqrt(np.maximum(lam, 0.0)), np.trace(B, axis1=-2, axis2=-1).real


def interaction(S, group_labels, form="ewald"):
    """(MIC [..., G, G], MIM [..., G, G], labels) for every pair of the groups np.unique(group_labels); symmetric, NaN diagonal."""
    group_labels = np.asarray(group_labels)
    labels = np.unique(group_labels)
    groups = [np.flatnonzero(group_labels == lab) for lab in labels]
    G = len(labels)
    lead = np.asarray(S).shape[:-2]
    mic, mim = np.full(lead + (G, G), np.nan), np.full(lead + (G, G), np.nan)
    for i in range(G):
        for j in range(i + 1, G):
            if form == "cholesky":
                c, m = interaction_cholesky(S, groups[i], groups[j])
            else:
                c, m = interaction_ewald(S, groups[i], groups[j])
            mic[..., i, j] = mic[..., j, i] = c
            mim[..., i, j] = mim[..., j, i] = m
    return mic, mim, labels
