"""NumPy float64 reference of the vectors that attain the maximized imaginary coherence (Ewald, Marzetti, Zappasodi, Meinecke &
Nolte 2012, NeuroImage 62:1964-1971; patterns: Haufe et al. 2014, NeuroImage 87:96-110), and the test spectrum of the device
tests.

Per pair of groups a, b of a Hermitian cross-spectral matrix S: R_g = Re S_gg, I = Im S_ab, D = R_a^-1/2 I R_b^-1/2 with
singular values sigma_1 >= sigma_2 >= ... and leading singular vectors u, v:
    filters   alpha = R_a^-1/2 u, beta = R_b^-1/2 v        (alpha^T R_a alpha = beta^T R_b beta = 1, alpha^T I beta = sigma_1 = MIC)
    patterns  a = R_a alpha, b = R_b beta                  (I beta = MIC a, I^T alpha = MIC b)
in two forms that share no factorisation:
  ewald     symmetric square roots of the real blocks (eigendecompositions) and the SVD of D;
  cholesky  the device's form: R_g = L_g L_g^T, M = L_a^-1 I L_b^-T, p the unit eigenvector of M M^T for lambda_max,
            q = M^T p / sigma_1, alpha = L_a^-T p, beta = L_b^-T q, a = L_a p, b = L_b q  (L_g^-1 R_g^1/2 is orthogonal).
One joint sign per pair is free; both forms fix it the same way: the entry of pattern a (the group with the lower label) with the
largest magnitude is positive, the lowest index on a tie.
"""
import numpy as np

from test_gpu_imaginary_interaction import var_spectrum      # (the well-conditioned VAR(1) spectrum of the MIC tests)


def _blocks(S, a, b):
    S = np.asarray(S, dtype=complex)
    a, b = np.asarray(a), np.asarray(b)
    return S[np.ix_(a, a)].real, S[np.ix_(b, b)].real, S[np.ix_(a, b)].imag


def _inv_sqrt(R):
    w, V = np.linalg.eigh(R)
    return (V / np.sqrt(w)) @ V.T


def apply_sign_rule(pattern_a, *vectors):
    """The vectors of one pair with the joint sign that makes the largest entry of ``pattern_a`` positive (np.argmax: the lowest
    index on a tie)."""
    k = int(np.argmax(np.abs(pattern_a)))
    s = -1.0 if pattern_a[k] < 0 else 1.0
    return tuple(s * v for v in vectors)


def pair_ewald(S, a, b):
    """(singular values of D, alpha, beta, pattern a, pattern b) of ONE matrix S [C, C] by symmetric whitening and an SVD."""
    Ra, Rb, I = _blocks(S, a, b)
    Wa, Wb = _inv_sqrt(Ra), _inv_sqrt(Rb)
    U, sv, Vt = np.linalg.svd(Wa @ I @ Wb)
    alpha, beta = Wa @ U[:, 0], Wb @ Vt[0]
    pa, pb = Ra @ alpha, Rb @ beta
    pa, pb, alpha, beta = apply_sign_rule(pa, pa, pb, alpha, beta)
    return sv, alpha, beta, pa, pb


def pair_cholesky(S, a, b):
    """The same of ONE matrix S [C, C] in the device's form (real Cholesky factors, eigenvector of M M^T)."""
    Ra, Rb, I = _blocks(S, a, b)
    La, Lb = np.linalg.cholesky(Ra), np.linalg.cholesky(Rb)
    M = np.linalg.solve(Lb, np.linalg.solve(La, I).T).T                 # L_a^-1 I L_b^-T
    lam, P = np.linalg.eigh(M @ M.T)
    p = P[:, -1]
    sv = np.sqrt(np.maximum(lam[::-1], 0.0))
    q = M.T @ p / sv[0]
    alpha, beta = np.linalg.solve(La.T, p), np.linalg.solve(Lb.T, q)
    pa, pb = La @ p, Lb @ q
    pa, pb, alpha, beta = apply_sign_rule(pa, pa, pb, alpha, beta)
    return sv, alpha, beta, pa, pb


def vectors(S, group_labels, form="ewald"):
    """Every bin and pair of groups of S [F, C, C]: dict with ``mic`` and ``sigma2`` (the second singular value, 0 when a group
    has one channel) [F, G, G], ``filters`` and ``patterns`` [F, G, G, n_max] laid out as the device lays them out (entry [a][b] is
    group a's vector in its interaction with b; NaN beyond the group's size and on the diagonal), ``labels`` and ``members``.
    A pair whose D is exactly 0 has MIC 0 and NaN vectors."""
    S = np.asarray(S)
    group_labels = np.asarray(group_labels)
    labels = np.unique(group_labels)
    members = [np.flatnonzero(group_labels == lab) for lab in labels]
    G, F, n_max = len(labels), S.shape[0], max(len(m) for m in members)
    mic, sigma2 = np.full((F, G, G), np.nan), np.full((F, G, G), np.nan)
    filters, patterns = np.full((F, G, G, n_max), np.nan), np.full((F, G, G, n_max), np.nan)
    one = pair_cholesky if form == "cholesky" else pair_ewald
    for f in range(F):
        for i in range(G):
            for j in range(i + 1, G):
                if not np.any(_blocks(S[f], members[i], members[j])[2]):
                    mic[f, i, j] = mic[f, j, i] = sigma2[f, i, j] = sigma2[f, j, i] = 0.0
                    continue
                sv, alpha, beta, pa, pb = one(S[f], members[i], members[j])
                mic[f, i, j] = mic[f, j, i] = sv[0]
                sigma2[f, i, j] = sigma2[f, j, i] = sv[1] if len(sv) > 1 else 0.0
                filters[f, i, j, :len(alpha)], filters[f, j, i, :len(beta)] = alpha, beta
                patterns[f, i, j, :len(pa)], patterns[f, j, i, :len(pb)] = pa, pb
    return dict(mic=mic, sigma2=sigma2, filters=filters, patterns=patterns, labels=labels, members=members)


def amplification(sigma1, sigma2):
    """max(1, 2 sigma_1 / (sigma_1^2 - sigma_2^2)): how much an error eps of MIC may turn the leading singular vectors, to first
    order -- d lambda <= 2 sigma_1 eps for lambda = sigma^2, sin(angle) <= d lambda / (lambda_1 - lambda_2)."""
    sigma1, sigma2 = np.asarray(sigma1, dtype=float), np.asarray(sigma2, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.maximum(1.0, 2.0 * sigma1 / (sigma1 ** 2 - sigma2 ** 2))


def relative_gap(sigma1, sigma2):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(sigma1) - np.asarray(sigma2)) / np.asarray(sigma1)


# ---- the test spectrum ------------------------------------------------------------------------------------------------------
def planted_spectrum(labels, seed, n_fft=32, pair=None):
    """Two-sided spectrum [n_fft, C, C] with ONE lagged interaction planted between two groups, so that sigma_1 is well separated
    from sigma_2 at every interior bin (the plain var_spectrum has relative gaps below 0.01 at 64 ... 128 channels):
        S(f) = 0.1 var_spectrum(C, seed) + (I + Q Q^T / 2) + 4 w(f) w(f)^H,   w(f) = g_a + g_b exp(-2 pi i f),
    Q = standard_normal((C, C)) / sqrt(C), g_a and g_b random unit vectors supported on the two groups of ``pair`` (indices into
    np.unique(labels); default the first two): group b sees the planted source one sample after group a.
    Returns (S, g_a [C], g_b [C])."""
    labels = np.asarray(labels)
    C = len(labels)
    uniq = np.unique(labels)
    ia, ib = (0, 1) if pair is None else pair
    rng = np.random.default_rng(seed + 1000)
    Q = rng.standard_normal((C, C)) / np.sqrt(C)
    g = []
    for lab in (uniq[ia], uniq[ib]):
        v = np.zeros(C)
        idx = np.flatnonzero(labels == lab)
        v[idx] = rng.standard_normal(len(idx))
        g.append(v / np.linalg.norm(v))
    f = np.arange(n_fft) / n_fft
    w = g[0][None, :] + g[1][None, :] * np.exp(-2j * np.pi * f)[:, None]
    S = 0.1 * var_spectrum(C, seed, n_fft) + (np.eye(C) + 0.5 * Q @ Q.T)[None] + 4.0 * w[:, :, None] * np.conj(w[:, None, :])
    return S, g[0], g[1]


# every tier edge of the MIC kernels, and the edge of the vector kernel's own split: up to 51 channels a pair keeps its blocks in
# LDS, from 52 on in the global scratch (sc_interaction_vectors_lds_group; the device tests assert that this is the edge)
LDS_EDGE = 51
GROUP_SIZES = [(1, 1), (1, 16), (2, 3), (16, 16), (16, 17), (32, 33), (51, 51), (51, 52), (64, 64), (64, 65), (96, 128), (128, 128)]


def size_case(sizes):
    """The spectrum of the group-size cases: permuted labels 0 / 1 of na / nb channels, seed na + nb.  Returns (S, labels, g_a, g_b)."""
    na, nb = sizes
    C = na + nb
    labels = np.r_[np.zeros(na, int), np.ones(nb, int)][np.random.default_rng(C).permutation(C)]
    S, ga, gb = planted_spectrum(labels, C)
    return S, labels, ga, gb
