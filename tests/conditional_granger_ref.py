"""NumPy float64 reference of conditional spectral Granger prediction (Geweke 1984; Ding, Chen & Bressler 2006,
"Granger causality: basic theory and application to neuroscience", section 3.3), built step by step from the explicit
normalisations, and the closed form the device computes.

For target x = i, source y = j and conditioning set z = every other signal:
  full model     S = Psi Psi^H (Wilson), Psi0 = Re mean_n Psi, H = Psi Psi0^-1, Sigma = Psi0 Psi0^T
  reduced model  the spectrum without row / column j, Phi, Phi0, G = Phi Phi0^-1, Sigma^r = Phi0 Phi0^T
  normalisation  variables ordered (x, y, z) / (x, z); P = P2 P1 makes the full innovation of x uncorrelated with y and z,
                 P1r does the same for the reduced model; H~ = H P^-1, G~ = G P1r^-1, G~ext = G~ with y's row and column of the
                 identity inserted, Q = G~ext^-1 H~
  measure        F_{y -> x | z}(f) = ln(Sigma~^r_xx / |Q_xx(f) Sigma~_xx Q_xx(f)^*|)
Output [..., n_freq = N/2+1, C, C], out[..., i, j] = j -> i given the rest, NaN on the diagonal and wherever the value is not
positive (the pairwise measure's convention); columns not dropped are NaN too.
"""
import numpy as np

from oracle.spectral_oracle import minimum_phase_decomposition


def _factor(S):
    """Wilson factor of [..., N, c, c] two-sided spectra (the oracle's iteration over a flat batch)."""
    lead, tail = S.shape[:-3], S.shape[-3:]
    G = minimum_phase_decomposition(S.reshape((-1,) + tail))
    return G.reshape(lead + tail)


def lag0(G):
    """Re mean over all N bins of the factor (= ifft(G)[0].real)."""
    return G.real.mean(axis=-3)


def _reduced(S, j):
    keep = [k for k in range(S.shape[-1]) if k != j]
    return S[..., keep, :][..., :, keep], keep


def var_spectrum(A, sigma, n_fft):
    """Exact two-sided spectrum S(f) = H(f) Sigma H(f)^H of x_t = sum_l A[l] x_{t-l-1} + e_t, e ~ N(0, sigma);
    A [p, C, C].  Bin n is the frequency n / n_fft (the device's FFT order)."""
    C = sigma.shape[0]
    f = np.arange(n_fft) / n_fft
    Af = np.eye(C)[None].astype(complex).repeat(n_fft, axis=0)
    for lag in range(A.shape[0]):
        Af = Af - A[lag][None] * np.exp(-2j * np.pi * f * (lag + 1))[:, None, None]
    H = np.linalg.inv(Af)
    return H @ sigma @ np.conj(np.swapaxes(H, -1, -2))


def conditional_granger_ding(S, dropped=None):
    """The explicit Ding et al. construction on two-sided spectra S [..., N, C, C]; ``dropped``: the sources j to compute
    (default all)."""
    S = np.asarray(S, dtype=complex)
    N, C = S.shape[-3], S.shape[-1]
    nn = np.arange(N // 2 + 1)
    out = np.full(S.shape[:-3] + (nn.size, C, C), np.nan)
    Psi = _factor(S)
    Psi0 = lag0(Psi)
    H = (Psi @ np.linalg.inv(Psi0)[..., None, :, :])[..., nn, :, :]
    Sigma = Psi0 @ np.swapaxes(Psi0, -1, -2)
    for j in (range(C) if dropped is None else dropped):
        Sr, keep = _reduced(S, j)
        Phi = _factor(Sr)
        Phi0 = lag0(Phi)
        Gr = (Phi @ np.linalg.inv(Phi0)[..., None, :, :])[..., nn, :, :]
        Sigr = Phi0 @ np.swapaxes(Phi0, -1, -2)
        for i in range(C):
            if i == j:
                continue
            rest = [k for k in range(C) if k not in (i, j)]
            order = [i, j] + rest                       # full model as (x, y, z)
            Hp = H[..., order, :][..., :, order]
            Sp = Sigma[..., order, :][..., :, order]
            nz = len(rest)
            # P1: x's innovation out of y and z; P2: then y's out of z
            P1 = np.broadcast_to(np.eye(C), Sp.shape).copy()
            P1[..., 1:, 0] = -Sp[..., 1:, 0] / Sp[..., :1, 0]
            S1 = P1 @ Sp @ np.swapaxes(P1, -1, -2)
            P2 = np.broadcast_to(np.eye(C), Sp.shape).copy()
            if nz:
                P2[..., 2:, 1] = -S1[..., 2:, 1] / S1[..., 1:2, 1]
            P = P2 @ P1
            Sig_t = P @ Sp @ np.swapaxes(P, -1, -2)
            H_t = Hp @ np.linalg.inv(P)[..., None, :, :]
            # reduced model as (x, z)
            r_order = [keep.index(i)] + [keep.index(k) for k in rest]
            Gp = Gr[..., r_order, :][..., :, r_order]
            Srp = Sigr[..., r_order, :][..., :, r_order]
            P1r = np.broadcast_to(np.eye(C - 1), Srp.shape).copy()
            P1r[..., 1:, 0] = -Srp[..., 1:, 0] / Srp[..., :1, 0]
            Sigr_t = P1r @ Srp @ np.swapaxes(P1r, -1, -2)
            G_t = Gp @ np.linalg.inv(P1r)[..., None, :, :]
            # G~ext: the reduced transfer function with y's row and column of the identity inserted
            Gext = np.zeros(G_t.shape[:-2] + (C, C), dtype=complex)
            idx = np.array([0] + list(range(2, C)))
            Gext[..., idx[:, None], idx[None, :]] = G_t
            Gext[..., 1, 1] = 1.0
            Q = np.linalg.inv(Gext) @ H_t
            q = Q[..., 0, 0]
            num = Sigr_t[..., 0, 0][..., None]
            den = np.abs(q * Sig_t[..., 0, 0][..., None] * np.conj(q))
            with np.errstate(invalid="ignore", divide="ignore"):
                val = np.log(num / den)
            val[~(val > 0)] = np.nan
            out[..., :, i, j] = val
    return out


def conditional_granger_closed(S, dropped=None):
    """The closed form of sc_conditional.hip on the same factors: ln(Sigma^r_ii Sigma_ii / |v_i|^2),
    v = Phi0 Phi^-1 (Psi Psi0^T)[rows != j, col i] at the row of i."""
    S = np.asarray(S, dtype=complex)
    N, C = S.shape[-3], S.shape[-1]
    nn = np.arange(N // 2 + 1)
    out = np.full(S.shape[:-3] + (nn.size, C, C), np.nan)
    Psi = _factor(S)
    Psi0 = lag0(Psi)
    M = Psi[..., nn, :, :] @ np.swapaxes(Psi0, -1, -2)[..., None, :, :]
    sig = np.einsum("...il,...il->...i", Psi0, Psi0)
    for j in (range(C) if dropped is None else dropped):
        Sr, keep = _reduced(S, j)
        Phi = _factor(Sr)
        Phi0 = lag0(Phi)
        sigr = np.einsum("...il,...il->...i", Phi0, Phi0)
        K = Phi0[..., None, :, :] @ np.linalg.inv(Phi[..., nn, :, :])
        V = K @ M[..., keep, :][..., :, keep]
        v = np.diagonal(V, axis1=-2, axis2=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            val = np.log(sigr[..., None, :] * sig[..., None, keep] / np.abs(v) ** 2)
        val[~(val > 0)] = np.nan
        out[..., keep, j] = val
    return out


def time_domain_conditional(S, dropped=None):
    """Geweke's time-domain value ln(Sigma^r_ii / Sigma_ii), [..., C, C] (out[..., i, j], NaN on the diagonal): the mean of
    the spectral measure over all N bins (the integral identity)."""
    S = np.asarray(S, dtype=complex)
    C = S.shape[-1]
    out = np.full(S.shape[:-3] + (C, C), np.nan)
    Psi0 = lag0(_factor(S))
    sig = np.einsum("...il,...il->...i", Psi0, Psi0)
    for j in (range(C) if dropped is None else dropped):
        Sr, keep = _reduced(S, j)
        Phi0 = lag0(_factor(Sr))
        sigr = np.einsum("...il,...il->...i", Phi0, Phi0)
        out[..., keep, j] = np.log(sigr / sig[..., keep])
    return out


def two_sided_mean(F_one_sided, n_fft):
    """Mean over all N bins of a measure of a real process, from its N/2+1 non-negative bins (F(-f) = F(f))."""
    F = np.asarray(F_one_sided)
    w = np.full(n_fft // 2 + 1, 2.0)
    w[0] = 1.0
    if n_fft % 2 == 0:
        w[-1] = 1.0
    return np.einsum("...fij,f->...ij", F, w) / n_fft


def coefficients_for(S):
    """Fourier coefficients [1, 1, K = C, N, C] whose taper average (expectation over tapers) equals S(f) exactly:
    coef[0, 0, k, n, c] = sqrt(C) R(n)[c, k] with R R^H = S (Cholesky)."""
    N, C = S.shape[0], S.shape[-1]
    R = np.linalg.cholesky(S)
    coef = np.sqrt(C) * np.transpose(R, (2, 0, 1))          # [K, N, C]: coef[k, n, c] = sqrt(C) R[n, c, k]
    return coef[None, None]
