"""Reference of the eight quantities sc_mvar_measure_f64 (csrc/sc_mvar.hip) derives from a minimum-phase factor
G [P][N][C][C] -- written from the reference's formulas (connectivity.py:567-589, :1237-1426, :1679-1748; the same as
oracle/spectral_oracle.py:376-445), NumPy only -- and builders of factors whose answers are known or hard.

    H0 = Re mean_n G[n]                              (the lag-0 coefficient: Re ifft_n(G)[0])
    Sigma = H0 H0^T                                  noise covariance
    H = G (H0 + lam I)^-1,  lam = 1e-12 mean(H0^2)   transfer function on the N // 2 + 1 non-negative bins; the mean runs over
                                                     every window (the reference's H0 carries the window axis)
    A = (H + lam' I)^-1, lam' = 1e-12 mean(|H|^2)    MVAR Fourier coefficients; the mean over every window and non-negative bin
    nv_i = Sigma_ii                                  the noise variance, indexed by the ROW channel in all five measures
    DTF  = |H_ij / sqrt(sum_j |H_ij|^2)|^2
    DC   = sqrt(nv_i) |H_ij|^2 / sqrt(sum_j nv_i |H_ij|^2)
    PDC  = |A_ij / sqrt(sum_i |A_ij|^2)|^2
    gPDC = |A_ij / sqrt(nv_i) / sqrt(sum_i |A_ij|^2 / nv_i)|^2
    dDTF = |H_ij / sqrt(sum_{f, j} |H_ij|^2)| sqrt(PDC_ij)        (f: the non-negative bins)

``evaluate(G, "float64")`` is the plain NumPy evaluation (np.linalg), ``evaluate(G, "extended")`` the same algebra in
np.longdouble / np.clongdouble with a batched Gauss-Jordan inverse (partial pivoting, vectorised over window and bin): 0.4 s at 70
signals, 1.8 s at 130, 16 s at 260 for 2 windows x 5 bins -- the device tests use it up to EXTENDED_MAX signals and the float64
evaluation above.  ``tikhonov=False`` leaves lam and lam' out: only to prove that a case is sensitive to them.
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52
EXTENDED_MAX = 132
TIKHONOV = 1e-12
# the order of _lib.MVAR_* (include/sc_hip.h: SC_MVAR_DTF ... SC_MVAR_NOISE_COVARIANCE)
QUANTITIES = ("directed_transfer_function", "directed_coherence", "partial_directed_coherence",
              "generalized_partial_directed_coherence", "direct_directed_transfer_function", "transfer_function",
              "mvar_coefficients", "noise_covariance")
MEASURES = QUANTITIES[:5]


def inverse_extended(M):
    """M^-1 of [..., C, C] matrices in extended precision: Gauss-Jordan on [M | I] with partial pivoting, every matrix of the
    batch one step at a time."""
    M = np.array(M, dtype=CLD if np.iscomplexobj(M) else LD)
    C = M.shape[-1]
    aug = np.concatenate([M, np.broadcast_to(np.eye(C, dtype=M.dtype), M.shape)], axis=-1).reshape(-1, C, 2 * C)
    idx = np.arange(aug.shape[0])
    for k in range(C):
        piv = k + np.argmax(np.abs(aug[:, k:, k]), axis=1)
        rk, rp = aug[idx, k].copy(), aug[idx, piv].copy()
        aug[idx, k], aug[idx, piv] = rp, rk
        aug[:, k] /= aug[:, k, k][:, None]
        f = aug[:, :, k].copy()
        f[:, k] = 0
        aug -= f[:, :, None] * aug[:, k][:, None, :]
    return aug[:, :, C:].reshape(M.shape)


def measures_from(H, A, sigma):
    """The five measures from H, A [P][F][C][C] and Sigma [P][C][C], in the precision of the arguments."""
    nv = np.diagonal(sigma, axis1=-1, axis2=-2)[..., np.newaxis, :, np.newaxis]         # (P, 1, C, 1): the row channel
    pH, pA = np.abs(H) ** 2, np.abs(A) ** 2
    pdc = np.abs(A / np.sqrt(pA.sum(axis=-2, keepdims=True))) ** 2
    return {
        "directed_transfer_function": np.abs(H / np.sqrt(pH.sum(axis=-1, keepdims=True))) ** 2,
        "directed_coherence": np.sqrt(nv) * pH / np.sqrt((nv * pH).sum(axis=-1, keepdims=True)),
        "partial_directed_coherence": pdc,
        "generalized_partial_directed_coherence": np.abs(A / np.sqrt(nv) / np.sqrt((pA / nv).sum(axis=-2, keepdims=True))) ** 2,
        "direct_directed_transfer_function": np.abs(H / np.sqrt(pH.sum(axis=(-1, -3), keepdims=True))) * np.sqrt(pdc),
    }


def evaluate(G, precision="float64", tikhonov=True):
    """{quantity: array} of the eight quantities of G [P][N][C][C] complex128 (``precision``: "float64" or "extended")."""
    G = np.asarray(G)
    assert G.ndim == 4 and G.shape[-1] == G.shape[-2] and precision in ("float64", "extended")
    ext = precision == "extended"
    real, cplx = (LD, CLD) if ext else (np.float64, np.complex128)
    inv = inverse_extended if ext else np.linalg.inv
    G = G.astype(cplx)
    N, C = G.shape[1], G.shape[-1]
    F = N // 2 + 1
    eye = np.eye(C, dtype=real)
    H0 = G.real.sum(axis=1) / real(N)
    lam = real(TIKHONOV) * np.mean(H0 * H0) if tikhonov else real(0)
    H = np.matmul(G[:, :F], inv(H0 + lam * eye).astype(cplx)[:, None])
    lam2 = real(TIKHONOV) * np.mean((np.conj(H) * H).real) if tikhonov else real(0)
    A = inv(H + lam2 * eye)
    sigma = np.matmul(H0, H0.swapaxes(-1, -2))
    out = measures_from(H, A, sigma)
    out.update(transfer_function=H, mvar_coefficients=A, noise_covariance=sigma)
    return out


def reference(G, tikhonov=True):
    """The evaluation the device tests compare with: extended up to EXTENDED_MAX signals, float64 beyond."""
    return evaluate(G, "extended" if G.shape[-1] <= EXTENDED_MAX else "float64", tikhonov)


def window_scale(ref):
    """max |ref| of every window, shaped to broadcast against ``ref`` (the first axis is the window)."""
    return np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (ref.ndim - 1))


def ratio(got, ref, scale=None):
    """max |got - ref| / (2^-52 max |ref|) with the maximum of ``ref`` taken per window: a quiet window is not judged on a
    loud one's scale.  (``scale``: per-window multipliers of the denominator.)  NaN or a wrong shape: infinite."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return np.inf
    den = EPS * window_scale(ref)
    if scale is not None:
        den = den * np.asarray(scale, dtype=den.dtype).reshape(den.shape)
    return float((np.abs(got.astype(ref.dtype) - ref) / den).max())


# ---- factors ----------------------------------------------------------------------------------------------------------------------
def _spectral_norm(rng, C, norm):
    B = rng.standard_normal((C, C))
    return B * (norm / np.linalg.norm(B, 2))


def _polynomial(B1, B2, N):
    """Hz[n] = I + B1 z + B2 z^2 at z = exp(-2 pi i n / N): [N][C][C]"""
    z = np.exp(-2j * np.pi * np.arange(N) / N)
    return np.eye(B1.shape[0])[None] + B1[None] * z[:, None, None] + B2[None] * (z ** 2)[:, None, None]


def structured_parts(C, N, P, seed):
    """The pieces of ``structured``: per window B1, B2 (spectral norms 0.5 and 0.25), L = chol(I + 0.5 M M^T) with
    M = randn / sqrt(C), d = 10^U(-1.5, 1.5) (1 + 3 p) and the column permutation."""
    rng = np.random.default_rng(seed)
    parts = []
    for p in range(P):
        B1, B2 = _spectral_norm(rng, C, 0.5), _spectral_norm(rng, C, 0.25)
        M = rng.standard_normal((C, C)) / np.sqrt(C)
        L = np.linalg.cholesky(np.eye(C) + 0.5 * M @ M.T)
        d = 10.0 ** rng.uniform(-1.5, 1.5, C) * (1 + 3 * p)
        parts.append(dict(B1=B1, B2=B2, L=L, d=d, perm=rng.permutation(C)))
    return parts


def structured(C, N, P, seed, closed=False):
    """G_p(z) = (I + B1 z + B2 z^2) L_p D_p Pi_p.  For N >= 3 the mean over the bins of z and z^2 vanishes, so H0 = L D Pi,
    H = I + B1 z + B2 z^2 and Sigma = L D^2 L^T without any inverse (``closed=True``: also returns them, in extended
    precision, as {"transfer_function", "noise_covariance"}); the noise variances span about five decades and differ per window,
    cond(H) is about 2.3, and gPDC differs from PDC by up to 0.9."""
    parts = structured_parts(C, N, P, seed)
    G = np.empty((P, N, C, C), np.complex128)
    for p, q in enumerate(parts):
        G[p] = _polynomial(q["B1"], q["B2"], N) @ (q["L"] * q["d"][None, :])[:, q["perm"]]
    if not closed:
        return G
    assert N >= 3
    F = N // 2 + 1
    Hc = np.stack([_polynomial(q["B1"].astype(LD), q["B2"].astype(LD), N)[:F] for q in parts])
    Sc = np.stack([np.matmul(q["L"].astype(LD) * (q["d"].astype(LD) ** 2)[None, :], q["L"].astype(LD).T) for q in parts])
    return G, {"transfer_function": Hc, "noise_covariance": Sc}


def free(C, N, P, seed):
    """An independent complex Gaussian matrix per bin (entries of variance 1 / C: spectral norm about 2) plus 3 I, Hermitian
    symmetric over the bins (G[N - n] = conj G[n], real at n = 0 and N / 2), window p scaled by 1 + 3 p.  Not a minimum-phase
    factor: the kernels are algebra on whatever they are given."""
    rng = np.random.default_rng(seed)
    G = np.empty((P, N, C, C), np.complex128)
    for p in range(P):
        X = (rng.standard_normal((N, C, C)) + 1j * rng.standard_normal((N, C, C))) / np.sqrt(2.0 * C)
        for n in range(N):
            m = (N - n) % N
            if m == n:
                X[n] = np.sqrt(2.0) * X[n].real
            elif m < n:
                X[n] = np.conj(X[m])
        G[p] = (X + 3.0 * np.eye(C)[None]) * (1 + 3 * p)
    return G


TIKHONOV_COND = 1e6
TIKHONOV_WINDOW = 0


def _orthogonal(rng, C, unitary):
    X = rng.standard_normal((C, C)) + (1j * rng.standard_normal((C, C)) if unitary else 0.0)
    return np.linalg.qr(X)[0]


def tikhonov(C, N, P, seed, where):
    """The ``structured`` factor with one matrix of window TIKHONOV_WINDOW replaced by U diag(1, ..., 1, 1e-6) V^H (U, V random
    orthogonal / unitary: condition number TIKHONOV_COND), where the lam terms move the answer far more than rounding does:

      where = "h0": H0 of the window (real; the other windows keep their large L D Pi, which set lam);
      where = "h" : H at the interior bin 1 of the window; bin 0 takes -2 Re of the change, so that the mean over the bins stays
                    I and H0 stays L D Pi."""
    assert where in ("h0", "h") and N >= 4
    parts = structured_parts(C, N, P, seed)
    rng = np.random.default_rng(seed + 77777)
    s = np.ones(C)
    s[-1] = 1.0 / TIKHONOV_COND
    G = np.empty((P, N, C, C), np.complex128)
    for p, q in enumerate(parts):
        Hz = _polynomial(q["B1"], q["B2"], N)
        H0 = (q["L"] * q["d"][None, :])[:, q["perm"]]
        if p == TIKHONOV_WINDOW and where == "h0":
            H0 = (_orthogonal(rng, C, False) * s[None, :]) @ _orthogonal(rng, C, False).T
        if p == TIKHONOV_WINDOW and where == "h":
            Hn = (_orthogonal(rng, C, True) * s[None, :]) @ np.conj(_orthogonal(rng, C, True)).T
            Hz[0] = Hz[0] - 2.0 * (Hn - Hz[1]).real
            Hz[1], Hz[N - 1] = Hn, np.conj(Hn)
        G[p] = Hz @ H0
    return G
