"""NumPy float64 reference of the vectors that attain canonical coherence and of its whole spectrum.

Per pair of groups a, b of a Hermitian cross-spectral matrix S, with D = S_aa^-1/2 S_ab S_bb^-1/2, singular values
rho_1 >= rho_2 >= ... (the canonical coherences; Connectivity.canonical_coherence and the oracle return rho_1^2) and leading
singular vectors u, v:
    filters   alpha = S_aa^-1/2 u, beta = S_bb^-1/2 v   (alpha^H S_aa alpha = beta^H S_bb beta = 1, alpha^H S_ab beta = rho_1)
    patterns  a = S_aa alpha, b = S_bb beta             (S_ab beta = rho_1 a, S_ab^H alpha = rho_1 b)
in two forms that share no factorisation:
  ewald     Hermitian inverse square roots of the group blocks (eigendecompositions) and the SVD of D;
  cholesky  the device's form: S_gg = L_g L_g^H, M = L_a^-1 S_ab L_b^-H, p the unit eigenvector of M M^H for lambda_max,
            q = M^H p / rho_1, alpha = L_a^-H p, beta = L_b^-H q, a = L_a p, b = L_b q  (L_g^-1 S_gg^1/2 is unitary).
One joint unit phase per pair is free; both forms fix it the same way: the entry of pattern a (the group with the lower label)
with the largest magnitude is real and positive, the lowest index on a tie.

The test spectrum is the planted spectrum of tests/interaction_vectors_ref.py as it stands: at every interior bin (1 ... 15) of
every size below rho_1 is 0.63 ... 0.75, the amplification max(1, 2 rho_1 / (rho_1^2 - rho_2^2)) at most 4.4, cond(S) <= 9.1.
"""
import numpy as np

from interaction_vectors_ref import amplification, planted_spectrum, size_case      # noqa: F401  (the tests take them from here)

# Up to LDS_EDGE channels a pair keeps its blocks in LDS, beyond in the global scratch: sc_canonical_vectors_lds_group, read off the
# built library (51 -> 51, 52 -> 51).  The four vectors are complex here, 4 KB more than the MIC vectors take, and the layout of
# 51 channels (156 508 bytes dynamic + 6 144 reserved = 162 652) still fits the 163 840 bytes: the edge is that of the MIC vectors.
LDS_EDGE = 51
GROUP_SIZES = [(1, 1), (1, 16), (2, 3), (16, 16), (16, 17), (32, 33), (LDS_EDGE, LDS_EDGE), (LDS_EDGE, LDS_EDGE + 1), (64, 64), (64, 65),
               (96, 128), (128, 128)]


def _blocks(S, a, b):
    S = np.asarray(S, dtype=complex)
    a, b = np.asarray(a), np.asarray(b)
    return S[np.ix_(a, a)], S[np.ix_(b, b)], S[np.ix_(a, b)]


def _inv_sqrt(R):
    w, V = np.linalg.eigh(R)
    return (V / np.sqrt(w)) @ V.conj().T


def apply_phase_rule(pattern_a, *vectors):
    """The vectors of one pair with the joint unit phase that makes the entry of largest magnitude of ``pattern_a`` real and
    positive (np.argmax: the lowest index on a tie)."""
    k = int(np.argmax(np.abs(pattern_a)))
    m = abs(pattern_a[k])
    ph = np.conj(pattern_a[k]) / m if m > 0 else 1.0
    return tuple(ph * v for v in vectors)


def pair_ewald(S, a, b):
    """(singular values of D, alpha, beta, pattern a, pattern b) of ONE matrix S [C, C] by Hermitian whitening and an SVD."""
    Sa, Sb, Sab = _blocks(S, a, b)
    Wa, Wb = _inv_sqrt(Sa), _inv_sqrt(Sb)
    U, sv, Vh = np.linalg.svd(Wa @ Sab @ Wb)
    alpha, beta = Wa @ U[:, 0], Wb @ Vh[0].conj()
    pa, pb = Sa @ alpha, Sb @ beta
    pa, pb, alpha, beta = apply_phase_rule(pa, pa, pb, alpha, beta)
    return sv, alpha, beta, pa, pb


def pair_cholesky(S, a, b):
    """The same of ONE matrix S [C, C] in the device's form (complex Cholesky factors, eigenvector of M M^H)."""
    Sa, Sb, Sab = _blocks(S, a, b)
    La, Lb = np.linalg.cholesky(Sa), np.linalg.cholesky(Sb)
    M = np.linalg.solve(Lb, np.linalg.solve(La, Sab).conj().T).conj().T          # L_a^-1 S_ab L_b^-H
    if M.shape[0] <= M.shape[1]:
        lam, P = np.linalg.eigh(M @ M.conj().T)
        p = P[:, -1]
        sv = np.sqrt(np.clip(lam[::-1], 0.0, None))
        q = M.conj().T @ p / sv[0]
    else:                                                                       # B on the smaller group's side
        lam, Q = np.linalg.eigh(M.conj().T @ M)
        q = Q[:, -1]
        sv = np.sqrt(np.clip(lam[::-1], 0.0, None))
        p = M @ q / sv[0]
    alpha, beta = np.linalg.solve(La.conj().T, p), np.linalg.solve(Lb.conj().T, q)
    pa, pb = La @ p, Lb @ q
    pa, pb, alpha, beta = apply_phase_rule(pa, pa, pb, alpha, beta)
    return sv, alpha, beta, pa, pb


def vectors(S, group_labels, form="ewald"):
    """Every bin and pair of groups of S [F, C, C]: dict with ``coherence`` [F, G, G] (rho_1), ``coherences`` [F, G, G, n_max]
    (descending, NaN beyond min(n_a, n_b)), complex ``filters`` and ``patterns`` [F, G, G, n_max] laid out as the device lays them
    out (entry [a][b] is group a's vector in its pairing with b; NaN beyond the group's size and on the diagonal), ``labels`` and
    ``members``.  A pair whose cross block is exactly 0 has coherences 0 and NaN vectors."""
    S = np.asarray(S)
    group_labels = np.asarray(group_labels)
    labels = np.unique(group_labels)
    members = [np.flatnonzero(group_labels == lab) for lab in labels]
    G, F, n_max = len(labels), S.shape[0], max(len(m) for m in members)
    coherence, coherences = np.full((F, G, G), np.nan), np.full((F, G, G, n_max), np.nan)
    filters, patterns = np.full((F, G, G, n_max), np.nan + 0j), np.full((F, G, G, n_max), np.nan + 0j)
    filters.imag = patterns.imag = np.nan
    one = pair_cholesky if form == "cholesky" else pair_ewald
    for f in range(F):
        for i in range(G):
            for j in range(i + 1, G):
                n_min = min(len(members[i]), len(members[j]))
                if not np.any(_blocks(S[f], members[i], members[j])[2]):
                    coherence[f, i, j] = coherence[f, j, i] = 0.0
                    coherences[f, i, j, :n_min] = coherences[f, j, i, :n_min] = 0.0
                    continue
                sv, alpha, beta, pa, pb = one(S[f], members[i], members[j])
                coherence[f, i, j] = coherence[f, j, i] = sv[0]
                coherences[f, i, j, :n_min] = coherences[f, j, i, :n_min] = sv[:n_min]
                filters[f, i, j, :len(alpha)], filters[f, j, i, :len(beta)] = alpha, beta
                patterns[f, i, j, :len(pa)], patterns[f, j, i, :len(pb)] = pa, pb
    return dict(coherence=coherence, coherences=coherences, filters=filters, patterns=patterns, labels=labels, members=members)


def second(coherences):
    """rho_2 [..., G, G] of ``coherences`` [..., G, G, n_max]: 0 where a group has one channel."""
    if coherences.shape[-1] < 2:
        return np.zeros(coherences.shape[:-1])
    return np.where(np.isnan(coherences[..., 1]), 0.0, coherences[..., 1])
