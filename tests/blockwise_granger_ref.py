"""NumPy float64 reference of blockwise spectral Granger prediction (Geweke 1982, "Measurement of linear dependence and
feedback between multiple time series", multivariate form) between blocks of signals, in three forms on the same Wilson factor.

For a pair of blocks a, b (n_a, n_b signals, m = n_a + n_b, ordered a first): S(f) the m x m two-sided spectrum, Psi(f) its
Wilson factor, Psi0 = Re mean_n Psi, Sigma = Psi0 Psi0^T, H = Psi Psi0^-1.
  (i)   Geweke's construction: P = [[I, 0], [-Sigma_ba Sigma_aa^-1, I]] makes the innovations of b uncorrelated with those of a,
        H~ = H P^-1, Sigma~ = P Sigma P^T (block diagonal: Sigma_aa, Sigma~_bb),
            F_{b -> a}(f) = ln det S_aa - ln det(H~_aa Sigma_aa H~_aa^H)        (S_aa = (H~ Sigma~ H~^H)_aa)
  (ii)  the reference form  ln det S_aa - ln det(S_aa - H_ab Sigma~_bb H_ab^H),  Sigma~_bb = Sigma_bb - Sigma_ba Sigma_aa^-1 Sigma_ab
  (iii) the null-space form of sc_blockwise.hip  ln det S_aa - ln det(S_aa - V_a V_a^H),  V_a = Psi[a, :] U_b, U_b the last n_b
        columns of the full Q of a QR of Psi0[a, :]^T
S_aa is the model spectrum (Psi Psi^H)_aa in (i) and the input spectrum in (ii) / (iii): they differ by the Wilson residual
(~1e-9 at the device's tolerance 1e-8; a tolerance of 1e-14 takes all three to rounding).
Output [..., n_freq = N/2+1, B, B], out[..., a, b] = b -> a, NaN on the diagonal, where a block is not positive definite and
where the value is not positive (the pairwise measure's convention).
"""
import numpy as np

from conditional_granger_ref import lag0
from oracle.spectral_oracle import minimum_phase_decomposition


def _factor(S, tolerance=1e-8):
    """Wilson factor of [..., N, c, c] two-sided spectra (the oracle's iteration over a flat batch; the device's tolerance by
    default -- a tighter one takes the factor to rounding, where the three forms agree to rounding too)."""
    lead, tail = S.shape[:-3], S.shape[-3:]
    G = minimum_phase_decomposition(S.reshape((-1,) + tail), tolerance=tolerance, max_iterations=200)
    return G.reshape(lead + tail)


def _ct(x):
    return np.conj(np.swapaxes(x, -1, -2))


def _logdet(M):
    """ln det of Hermitian matrices [..., n, n]; NaN where not positive definite."""
    M = 0.5 * (M + _ct(M))
    ok = np.linalg.eigvalsh(M)[..., 0] > 0
    _, ld = np.linalg.slogdet(np.where(ok[..., None, None], M, np.eye(M.shape[-1])))
    return np.where(ok, ld.real, np.nan)


def _clean(val):
    val = np.array(val, dtype=float)
    val[~(val > 0)] = np.nan
    return val


def _pair(S, ia, ib):
    idx = np.concatenate([ia, ib])
    return S[..., idx, :][..., :, idx]


def pair_geweke(S2, na, tolerance=1e-8):
    """(i): (F_{b -> a}, F_{a -> b}) [..., N/2+1] of one pair spectrum S2 [..., N, m, m] (a = the first na signals)."""
    N = S2.shape[-3]
    nn = np.arange(N // 2 + 1)
    Psi = _factor(S2, tolerance)
    Psi0 = lag0(Psi)
    H = (Psi @ np.linalg.inv(Psi0)[..., None, :, :])[..., nn, :, :]
    Sigma = Psi0 @ np.swapaxes(Psi0, -1, -2)
    out = []
    for t, o in ((slice(0, na), slice(na, None)), (slice(na, None), slice(0, na))):
        order = np.r_[np.arange(S2.shape[-1])[t], np.arange(S2.shape[-1])[o]]
        Hp, Sp = H[..., order, :][..., :, order], Sigma[..., order, :][..., :, order]
        nt = len(np.arange(S2.shape[-1])[t])
        P = np.broadcast_to(np.eye(len(order)), Sp.shape).copy()
        P[..., nt:, :nt] = -Sp[..., nt:, :nt] @ np.linalg.inv(Sp[..., :nt, :nt])
        Sig_t = P @ Sp @ np.swapaxes(P, -1, -2)
        H_t = Hp @ np.linalg.inv(P)[..., None, :, :]
        model = H_t @ Sig_t[..., None, :, :] @ _ct(H_t)
        own = H_t[..., :nt, :nt] @ Sig_t[..., None, :nt, :nt] @ _ct(H_t[..., :nt, :nt])
        out.append(_logdet(model[..., :nt, :nt]) - _logdet(own))
    return out[0], out[1]


def pair_reference(S2, na, tolerance=1e-8):
    """(ii)."""
    N = S2.shape[-3]
    nn = np.arange(N // 2 + 1)
    Psi = _factor(S2, tolerance)
    Psi0 = lag0(Psi)
    H = (Psi @ np.linalg.inv(Psi0)[..., None, :, :])[..., nn, :, :]
    Sigma = Psi0 @ np.swapaxes(Psi0, -1, -2)
    Sf = S2[..., nn, :, :]
    out = []
    for t, o in ((slice(0, na), slice(na, None)), (slice(na, None), slice(0, na))):
        St = Sigma[..., o, o] - Sigma[..., o, t] @ np.linalg.inv(Sigma[..., t, t]) @ Sigma[..., t, o]
        Hto = H[..., t, o]
        out.append(_logdet(Sf[..., t, t]) - _logdet(Sf[..., t, t] - Hto @ St[..., None, :, :] @ _ct(Hto)))
    return out[0], out[1]


def nullspace_basis(Psi0, rows):
    """Orthonormal basis of the null space of the rows Psi0[..., rows, :]: the last m - len(rows) columns of the full Q."""
    k = Psi0[..., rows, :].shape[-2]
    Q, _ = np.linalg.qr(np.swapaxes(Psi0[..., rows, :], -1, -2), mode="complete")
    return Q[..., :, k:]


def pair_nullspace(S2, na, tolerance=1e-8):
    """(iii)."""
    N, m = S2.shape[-3], S2.shape[-1]
    nn = np.arange(N // 2 + 1)
    Psi = _factor(S2, tolerance)
    Psi0 = lag0(Psi)
    Sf = S2[..., nn, :, :]
    out = []
    for t, o in ((slice(0, na), slice(na, m)), (slice(na, m), slice(0, na))):
        U = nullspace_basis(Psi0, t)                            # orthogonal to the rows of the target block
        V = Psi[..., nn, t, :] @ U[..., None, :, :]
        out.append(_logdet(Sf[..., t, t]) - _logdet(Sf[..., t, t] - V @ _ct(V)))
    return out[0], out[1]


FORMS = {"geweke": pair_geweke, "reference": pair_reference, "nullspace": pair_nullspace}


def blockwise_granger(S, group_labels, form="nullspace", tolerance=1e-8):
    """All ordered block pairs of two-sided spectra S [..., N, C, C]; blocks = np.unique(group_labels).  Returns
    (values [..., N/2+1, B, B], labels)."""
    S = np.asarray(S, dtype=complex)
    group_labels = np.asarray(group_labels)
    labels = np.unique(group_labels)
    blocks = [np.flatnonzero(group_labels == lab) for lab in labels]
    B, N = len(blocks), S.shape[-3]
    out = np.full(S.shape[:-3] + (N // 2 + 1, B, B), np.nan)
    for a in range(B):
        for b in range(a + 1, B):
            ba, ab = FORMS[form](_pair(S, blocks[a], blocks[b]), len(blocks[a]), tolerance)
            out[..., a, b], out[..., b, a] = _clean(ba), _clean(ab)
    return out, labels


def time_domain_blockwise(S, ia, ib):
    """Geweke's time-domain F_{b -> a} = ln(det Sigma_aa^(a alone) / det Sigma_aa): Sigma_aa of the joint model, Sigma_aa^(a alone)
    of the factor of S_aa alone."""
    S2 = _pair(np.asarray(S, dtype=complex), ia, ib)
    na = len(ia)
    Psi0 = lag0(_factor(S2))
    Sigma = Psi0 @ np.swapaxes(Psi0, -1, -2)
    Phi0 = lag0(_factor(S2[..., :na, :na]))
    alone = Phi0 @ np.swapaxes(Phi0, -1, -2)
    return np.linalg.slogdet(alone)[1] - np.linalg.slogdet(Sigma[..., :na, :na])[1]


def embed(core_S, core_labels, sizes, seed):
    """A spectrum of sum(sizes) signals whose blockwise Granger equals that of ``core_S`` [N, c, c] (block labels
    ``core_labels`` in 0 .. len(sizes)-1): the core signals at scattered places of their blocks, every other signal an
    independent AR(1) process of its own, then a random invertible mixing inside every block, S -> T S T^H with
    T = blockdiag(A_0, A_1, ...) -- adding independent processes and mixing inside blocks leave Geweke's measure unchanged.
    Returns (S [N, C, C], labels [C])."""
    rng = np.random.default_rng(seed)
    N = core_S.shape[0]
    core_labels = np.asarray(core_labels)
    C = int(sum(sizes))
    labels = np.concatenate([np.full(n, k) for k, n in enumerate(sizes)])
    perm = rng.permutation(C)                      # blocks interleaved over the signal axis
    labels = labels[perm]
    S = np.zeros((N, C, C), dtype=complex)
    place = []
    for k in range(len(sizes)):
        members = np.flatnonzero(labels == k)
        n_core = int((core_labels == k).sum())
        place.append(rng.choice(members, size=n_core, replace=False))
    core_pos = np.empty(len(core_labels), dtype=int)
    for k in range(len(sizes)):
        core_pos[core_labels == k] = place[k]
    S[:, core_pos[:, None], core_pos[None, :]] = core_S
    f = np.arange(N) / N
    for i in np.setdiff1d(np.arange(C), core_pos):
        phi = rng.uniform(-0.4, 0.4)
        S[:, i, i] = rng.uniform(0.7, 1.4) / np.abs(1 - phi * np.exp(-2j * np.pi * f)) ** 2
    T = np.zeros((C, C))
    for k in range(len(sizes)):
        members = np.flatnonzero(labels == k)
        n = len(members)
        A = np.eye(n) + 0.2 * rng.standard_normal((n, n)) / np.sqrt(n)
        T[members[:, None], members[None, :]] = A
    return T @ S @ T.T, labels
