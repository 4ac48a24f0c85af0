"""NumPy float64 reference of partial and multiple coherence GIVEN a chosen set of signals, in two forms that share no step.

With Z = ``given`` (m signals) and A = ``kept`` (a signals, disjoint from Z), both forms return (partial coherency given Z
complex128 [..., a, a] with a NaN diagonal, in the order of ``kept``; multiple coherence given Z float64 [..., a]):

    schur      from the cross-spectral matrices S [..., C, C]: E = S_AA - S_AZ S_ZZ^-1 S_ZA (partial_coherence_ref._schur), then
               E_ij / sqrt(E_ii E_jj) and sqrt(max(0, 1 - E_ii / S_ii))
    residuals  from the Fourier coefficients X [..., K, C] (K observations of C signals per bin): np.linalg.lstsq of the kept
               coefficients on the given ones, then the ordinary coherency of the residual coefficients e and
               sqrt(max(0, 1 - |e_i|^2 / |x_i|^2))
"""
import numpy as np

import partial_coherence_ref as pref


def _finish(E, s_kept):
    a = E.shape[-1]
    e = np.einsum("...ii->...i", E).real
    gamma = E / np.sqrt(e[..., :, None] * e[..., None, :])
    gamma[..., np.arange(a), np.arange(a)] = np.nan
    return gamma, np.sqrt(np.maximum(0.0, 1.0 - e / s_kept))


def schur(S, kept, given):
    S = np.asarray(S, dtype=complex)
    kept, given = [int(k) for k in kept], [int(k) for k in given]
    E = pref._schur(S, kept, given)
    return _finish(E, np.einsum("...ii->...i", S).real[..., kept])


def residuals(X, kept, given):
    X = np.asarray(X, dtype=complex)
    kept, given = [int(k) for k in kept], [int(k) for k in given]
    lead = X.shape[:-2]
    a = len(kept)
    gamma = np.empty(lead + (a, a), dtype=complex)
    multiple = np.empty(lead + (a,))
    for idx in np.ndindex(*lead):
        Xa, Xz = X[idx][:, kept], X[idx][:, given]
        beta = np.linalg.lstsq(Xz, Xa, rcond=None)[0]
        e = Xa - Xz @ beta                                       # [K, a] residual coefficients
        E = e.T @ np.conj(e)                                     # E_ij = sum_k e_i conj(e_j) (the common 1 / K cancels)
        p = np.einsum("ii->i", E).real
        g = E / np.sqrt(p[:, None] * p[None, :])
        g[np.arange(a), np.arange(a)] = np.nan
        gamma[idx] = g
        multiple[idx] = np.sqrt(np.maximum(0.0, 1.0 - p / (np.abs(Xa) ** 2).sum(axis=0)))
    return gamma, multiple


def conditioning(S, kept, given):
    """(largest condition number of the unit-diagonal given block, smallest residual share r_i = E_ii / S_ii) over the
    matrices of S: what the device's Cholesky and its residual test see."""
    S = np.asarray(S, dtype=complex)
    kept, given = [int(k) for k in kept], [int(k) for k in given]
    d = np.einsum("...ii->...i", S).real
    Z = S[..., given, :][..., :, given] / np.sqrt(d[..., given, None] * d[..., None, given])
    E = pref._schur(S, kept, given)
    r = np.einsum("...ii->...i", E).real / d[..., kept]
    return float(np.linalg.cond(Z).max()), float(r.min())
