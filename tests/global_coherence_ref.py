"""Reference for the global-coherence eigensolvers (sc_global_coherence_f64, csrc/sc_global.hip) on records built by hand: Hermitian
matrices whose eigen-decomposition is known without rounding, Wishart matrices, the special structures that steer the Householder
kernel into its branches, the record they are packed into, and the four checks of a result in extended precision.  NumPy only.

    exact(C, seed)            blocks D H Lambda H^T D^H / n (H: Hadamard, D: powers of i, Lambda: integers): float32 holds every entry
    free(C, n_obs, seed)      X^H X / n_obs of complex Gaussian coefficients with unequal channel gains; rank n_obs when n_obs < C
    SPECIAL[name](C)          dead channel, real tridiagonal, imaginary sub-diagonal, c I, 1 1^T, two identical blocks
    record(mats, n_obs, ...)  the accumulator record holding n_obs x mats and the two-sided stack a consumer must see
    check(A, values, ...)     values, residual, Gram and phase errors of a result, in units of 2^-52 ||A||_2 (2^-52 for the last two)

The bars of the three accuracy checks are K_VALUES, K_RESIDUAL and K_GRAM below: 8 x the worst ratio numpy.linalg.eigh reaches over
the cases of ``cases_a`` (tools/global_coherence_accuracy.py --cpu prints them; profiles/global_coherence_accuracy.txt), rounded up
to a power of two.  No device number enters them.
"""
import functools
from types import SimpleNamespace

import numpy as np

import epilogue_ref as eref

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52

# tools/global_coherence_accuracy.py --cpu, last line (profiles/global_coherence_accuracy.txt):
#             max     27.49     18.29     17.06      0.29
#   K = 8 x the NumPy maximum, rounded up to a power of two: values 256, residual 256, Gram 256
# (values: 27.49 is the ``free`` family at 512 signals, where the reference is numpy.linalg.eigvalsh with an error of its own; against
#  the known integers of the ``exact`` family NumPy stays below 17)
K_VALUES, K_RESIDUAL, K_GRAM = 256.0, 256.0, 256.0
# The phase rule makes one component real: v_m x conj(v_m) / |v_m| / ||v||.  Its imaginary part is Re v_m Im p + Im v_m Re p with
# p = conj(v_m) / (|v_m| ||v||): two products that cancel before rounding.  Each part of p carries two roundings (quotient, scale), each
# product one more: 6 x 2^-53 |Re v_m Im v_m| / |v_m| <= 3 x 2^-53 |v_m| in all, under 4 x 2^-52 (|v_m| <= 1).
K_PHASE = 4.0
# the parallel Jacobi kernels stop at off^2 <= 1e-28 dia^2 (global_coherence_kernel; gc_jacobi in csrc/sc_jacobi.h: total - dia <=
# 1e-28 dia), so a column of A V - V diag(lambda) = V (off-diagonal part of the rotated matrix) is at most 1e-14 ||A||_F long; x 2
JACOBI_RESIDUAL = 2e-14

SIZES_JACOBI = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32)                  # global_coherence_kernel (matrix and vectors in LDS)
SIZES_EIGH256 = (33, 34, 63, 64, 65, 127, 128, 129, 255, 256)       # global_coherence_eigh_kernel<256>
SIZES_EIGH512 = (257, 300, 511, 512)                                # global_coherence_eigh_kernel<512>
SIZES = SIZES_JACOBI + SIZES_EIGH256 + SIZES_EIGH512
FAMILIES = ("exact", "free")
N_OBS = 8                                                           # of the records of (a): a power of two, the division is exact

_RE, _IM = np.array([1.0, 0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0, -1.0])   # i^k


def hadamard(n):
    """The Sylvester matrix of order n = 2^k: entries +-1, H H^T = n I."""
    assert n >= 1 and n & (n - 1) == 0
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def blocks_of(C):
    """The powers of two of the binary expansion of C, largest first."""
    return [1 << b for b in range(C.bit_length() - 1, -1, -1) if C >> b & 1]


def distinct_integers(C, seed):
    """C different integers in 1 ... 4095 (eigenvalues at least 2^-12 ||A|| apart: closer than the kernel's cluster threshold)"""
    return np.random.default_rng(seed).choice(np.arange(1, 4096), size=C, replace=False).astype(np.float64)


def with_multiplicities(C, seed, mults=(2, 4, 16)):
    """Integers below 2^12 in which one value each is repeated 2, 4 and 16 times (as many of them as C has room for)"""
    base = list(distinct_integers(C, seed))
    out = []
    for m in mults:
        if len(out) + m <= C:
            out += [base.pop()] * m
    return np.array(out + base[:C - len(out)])


def graded(C):
    """2^0 ... 2^-40 in C steps of whole powers of two (repeats where C > 41)"""
    return 2.0 ** -np.round(np.linspace(0.0, 40.0, C))


def exact(C, seed, eigenvalues=None, scale=1.0):
    """A Hermitian C x C matrix with a known decomposition.  C is split into the power-of-two blocks of its binary expansion; a block
    of order n is D H Lambda H^T D^H / n with H the +-1 Hadamard matrix, D a random diagonal of powers of i and Lambda a diagonal of
    the given eigenvalues (default: distinct integers below 2^12; any multiset of C non-negative dyadic numbers, shuffled over the
    blocks).  Every entry is a sum of n signed eigenvalues over n -- with integers below 2^12 and n <= 512 a dyadic rational of at most
    21 bits, which float32 holds --, times a power of i.  One random permutation of the channels hides the blocks.  ``scale``: a common
    power of two.  Returns A [C, C] complex128, ``values`` [C] (of column k), ``U`` [C, C] (entries 0, +-1, +-i: column k is the
    UNNORMALISED eigenvector, A U[:, k] = values[k] U[:, k] without rounding) and ``n`` [C] (its squared norm, the block order)."""
    rng = np.random.default_rng(seed)
    lam = distinct_integers(C, seed + 7) if eigenvalues is None else np.asarray(eigenvalues, dtype=np.float64)
    assert lam.shape == (C,) and (lam >= 0).all()
    assert np.frexp(scale)[0] == 0.5, "scale must be a power of two"
    lam = rng.permutation(lam)
    re, im = np.zeros((C, C)), np.zeros((C, C))
    ure, uim = np.zeros((C, C)), np.zeros((C, C))
    order = np.zeros(C)
    o = 0
    for n in blocks_of(C):
        H = hadamard(n)
        k = rng.integers(0, 4, n)
        M = (H * lam[o:o + n]) @ H.T / n                  # whole multiples of the smallest eigenvalue's last bit: no rounding
        ph = (k[:, None] - k[None, :]) % 4
        s = slice(o, o + n)
        re[s, s], im[s, s] = M * _RE[ph], M * _IM[ph]
        ure[s, s], uim[s, s] = H * _RE[k][:, None], H * _IM[k][:, None]
        order[s] = n
        o += n
    perm = rng.permutation(C)
    A = eref.as_complex(re[np.ix_(perm, perm)] * scale, im[np.ix_(perm, perm)] * scale) + 0.0     # (+ 0.0: no negative zeros)
    return SimpleNamespace(A=A, values=lam * scale, U=eref.as_complex(ure[perm], uim[perm]), n=order)


def free(C, n_obs, seed):
    """X^H X / n_obs for X [n_obs, C] of complex Gaussian coefficients with channel gains 2^-2 ... 2^2: the cross-spectral matrix of
    n_obs observations, exactly Hermitian, of rank min(n_obs, C)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n_obs, C)) + 1j * rng.standard_normal((n_obs, C))) * np.sqrt(0.5) * 2.0 ** rng.uniform(-2.0, 2.0, C)
    A = X.conj().T @ X / n_obs
    A = 0.5 * (A + A.conj().T)
    A[np.arange(C), np.arange(C)] = A[np.arange(C), np.arange(C)].real
    return A


def _tridiagonal(d, e):
    return (np.diag(d) + np.diag(e, -1) + np.diag(np.conj(e), 1)).astype(np.complex128)


def dead_channel(C):
    """diag(1/4, 2/4, ...) with a zero at C / 2: every reflection is the identity, one eigenvalue is exactly 0"""
    d = (np.arange(C) + 1.0) / 4.0
    d[C // 2] = 0.0
    return np.diag(d).astype(np.complex128)


def real_tridiagonal(C):
    """diagonally dominant (positive definite), already in the form the reduction produces: the tail of every column is zero"""
    return _tridiagonal(3.0 + (np.arange(C) % 3), 0.25 + 0.75 * ((np.arange(C - 1) * 5 % 7) / 7.0))


def imaginary_subdiagonal(C):
    """the same with i e below the diagonal: tail zero, head imaginary -- a reflection with nothing but its phase"""
    return _tridiagonal(3.0 + (np.arange(C) % 3), 1j * (0.25 + 0.75 * ((np.arange(C - 1) * 5 % 7) / 7.0)))


def scaled_identity(C):
    return 3.0 * np.eye(C, dtype=np.complex128)


def rank_one(C):
    return np.ones((C, C), dtype=np.complex128)


def two_blocks(C):
    """diag(B, B) with B an ``exact`` matrix of order C / 2: every eigenvalue twice, one identity reflection between the blocks"""
    assert C % 2 == 0
    B = exact(C // 2, 4000 + C).A
    A = np.zeros((C, C), dtype=np.complex128)
    A[:C // 2, :C // 2] = A[C // 2:, C // 2:] = B
    return A


SPECIAL = {"dead_channel": dead_channel, "real_tridiagonal": real_tridiagonal, "imaginary_subdiagonal": imaginary_subdiagonal,
           "scaled_identity": scaled_identity, "rank_one": rank_one, "two_blocks": two_blocks}


def record(mats, n_obs, dtype, two_sided):
    """(record, stack): ``mats`` [n_groups, F, C, C] Hermitian, a matrix per (group, accumulated bin).  The record [n_groups F,
    floats_per_bin] of ``dtype`` holds the entries i <= j of n_obs x mats in the layout of include/sc_hip.h (SC_PLANE_CSM alone;
    tests/epilogue_ref.pack_record).  ``two_sided``: F = N, every bin its own matrix; otherwise F = N / 2 + 1 with N = 2 (F - 1) and
    bin n > N / 2 is the conjugate of bin N - n.  ``stack`` [n_groups, N, C, C] complex128 is what a consumer must see: the stored
    numbers (after the cast to ``dtype``) divided by n_obs -- ``mats`` itself when n_obs is a power of two and ``dtype`` holds them."""
    mats = np.asarray(mats, dtype=np.complex128)
    G, F, C, _ = mats.shape
    assert np.array_equal(mats, mats.conj().swapaxes(-1, -2)), "not exactly Hermitian"
    N = F if two_sided else 2 * (F - 1)
    assert two_sided or F != N, "F = N / 2 + 1 = N (N = 2) is read as two-sided"
    with np.errstate(over="ignore"):
        re, im = (mats.real * n_obs).astype(dtype), (mats.imag * n_obs).astype(dtype)
    rec = eref.pack_record({"s": eref.as_complex(re, im).reshape(G * F, C, C)}, C, eref.PLANE_CSM, dtype)
    seen = eref.as_complex(re.astype(np.float64) / n_obs, im.astype(np.float64) / n_obs)
    stack = np.empty((G, N, C, C), dtype=np.complex128)
    for n in range(N):
        stack[:, n] = seen[:, n] if two_sided or n <= N // 2 else seen[:, N - n].conj()
    return rec, stack


def unpack(rec, C, n_groups, n_obs):
    """[n_groups, F, C, C] complex128 from a record: the inverse of ``record`` (upper triangle mirrored, real diagonal)"""
    lay = eref.layout(C, eref.PLANE_CSM)
    tiles = np.asarray(rec, dtype=np.float64).reshape(rec.shape[0], 2, lay.n_tiles, eref.TILE, eref.TILE)
    P = lay.NB * eref.TILE
    full = np.zeros((rec.shape[0], 2, P, P))
    for bi in range(lay.NB):
        for bj in range(bi, lay.NB):
            full[:, :, bi * 16:(bi + 1) * 16, bj * 16:(bj + 1) * 16] = tiles[:, :, lay.tile_index(bi, bj)]
    up = np.triu(np.ones((C, C), dtype=bool))
    re = np.where(up, full[:, 0, :C, :C], full[:, 0, :C, :C].swapaxes(-1, -2)) / n_obs
    im = np.where(up, full[:, 1, :C, :C], -full[:, 1, :C, :C].swapaxes(-1, -2)) / n_obs
    im[:, np.arange(C), np.arange(C)] = 0.0
    return eref.as_complex(re, im).reshape(n_groups, -1, C, C)


# ---- products without rounding -----------------------------------------------------------------------------------------------------
_BITS = 21


def _slices(x):
    """x = q0 + q1 + q2 + (less than 2^-63 max |x|) with every q a whole multiple of its own power of two, below 2^21 of them: a
    float64 product of two slices summed over up to 2^11 terms is exact in any order"""
    x = np.asarray(x, dtype=np.float64)
    m = float(np.abs(x).max()) if x.size else 0.0
    if m == 0.0:
        return [x]
    s = 2.0 ** (np.frexp(m)[1] - _BITS)
    out, r = [], x
    for _ in range(3):
        q = np.round(r / s) * s
        out.append(q)
        r = r - q
        s *= 2.0 ** -_BITS
    return out


def matmul_ld(X, Y):
    """X @ Y in np.longdouble for float64 matrices: both are cut into three slices of 21 bits, the six products of slices that
    matter (the others are below 2^-63 of the product of the maxima) are exact float64 matrix products, and they are added in
    extended precision, smallest first."""
    assert X.shape[-1] == Y.shape[0] <= 2048
    xs, ys = _slices(X), _slices(Y)
    out = np.zeros((X.shape[0], Y.shape[1]), dtype=LD)
    for order in (2, 1, 0):
        for i in range(order + 1):
            if i < len(xs) and order - i < len(ys):
                out += (xs[i] @ ys[order - i]).astype(LD)
    return out


def cmatmul_ld(X, Y):
    """(real, imaginary) parts of X @ Y in np.longdouble for complex128 matrices"""
    X, Y = np.asarray(X, dtype=np.complex128), np.asarray(Y, dtype=np.complex128)
    m, k = X.shape[0], Y.shape[1]
    P = matmul_ld(np.concatenate([X.real, X.imag], axis=0), np.concatenate([Y.real, Y.imag], axis=1))
    return P[:m, :k] - P[m:, k:], P[:m, k:] + P[m:, :k]


def reference_values(A, exact_values=None):
    """every eigenvalue, largest first: the known ones, or numpy.linalg.eigvalsh"""
    v = np.asarray(exact_values, dtype=np.float64) if exact_values is not None else np.linalg.eigvalsh(A)
    return np.sort(v)[::-1]


def check(A, values, vectors, ascending, exact_values=None):
    """The four ratios of a result (values [K], vectors [C, K]) for the Hermitian matrix A, evaluated in np.longdouble:

      values    max_k |values[k] - reference| / (2^-52 ||A||_2); the reference is the k-th largest of ``exact_values`` or of
                numpy.linalg.eigvalsh(A), in the order ``ascending`` asks for
      residual  max_k ||A v_k - values[k] v_k||_2 / (2^-52 ||A||_2)
      gram      ||V^H V - I||_max / 2^-52   (with the residual this is the right statement about a repeated eigenvalue, where any
                orthonormal basis of the eigenspace is correct)
      phase     |Im v_m| / 2^-52 for the component of largest modulus, which must be positive; where several components share the
                largest modulus to 2^-40 (the ``exact`` family: all of a block) the one the solver chose counts

    Requires every output finite and every value >= 0."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no extended precision here: no reference"
    A = np.asarray(A, dtype=np.complex128)
    values, vectors = np.asarray(values, dtype=np.float64), np.asarray(vectors, dtype=np.complex128)
    C, K = vectors.shape
    assert A.shape == (C, C) and values.shape == (K,) and 1 <= K <= C
    assert np.isfinite(values).all() and np.isfinite(vectors.real).all() and np.isfinite(vectors.imag).all(), "non-finite output"
    assert (values >= 0).all(), f"negative value {values.min()}"
    ref = reference_values(A, exact_values)
    norm = LD(np.abs(ref).max())
    assert norm > 0
    top = ref[:K][::-1] if ascending else ref[:K]
    unit = LD(EPS) * norm
    r_values = float(np.abs(values.astype(LD) - top.astype(LD)).max() / unit)
    re, im = cmatmul_ld(A, vectors)
    re -= vectors.real.astype(LD) * values.astype(LD)
    im -= vectors.imag.astype(LD) * values.astype(LD)
    r_residual = float(np.sqrt((re * re + im * im).sum(axis=0)).max() / unit)
    gre, gim = cmatmul_ld(vectors.conj().T, vectors)
    gre -= np.eye(K, dtype=LD)
    r_gram = float(np.sqrt(gre * gre + gim * gim).max() / LD(EPS))
    mod = np.abs(vectors)
    r_phase = 0.0
    for k in range(K):
        near = np.flatnonzero(mod[:, k] >= mod[:, k].max() * (1.0 - 2.0 ** -40))
        real = near[vectors[near, k].real > 0]
        assert real.size, f"vector {k}: no component of largest modulus has a positive real part"
        r_phase = max(r_phase, float(np.abs(vectors[real, k].imag).min() / EPS))
    return {"values": r_values, "residual": r_residual, "gram": r_gram, "phase": r_phase}


BARS = {"values": K_VALUES, "residual": K_RESIDUAL, "gram": K_GRAM, "phase": K_PHASE}


def over_the_bars(ratios, bars=None):
    """{check: ratio} of the ratios above their bars"""
    bars = bars or BARS
    return {k: v for k, v in ratios.items() if not v <= bars[k]}


# ---- the cases of (a) --------------------------------------------------------------------------------------------------------------
def shape_a(C):
    """(n_groups, N, F) of the cases of (a): two windows of N = 4 from F = 3 accumulated bins; one window, N = F = 2 from 257 signals"""
    return (1, 2, 2) if C >= 257 else (2, 4, 3)


@functools.lru_cache(maxsize=4)
def cases_a(family, C):
    """(mats [n_groups, F, C, C], exact values [n_groups, F, C] or None): a different matrix in every (group, bin); never written to"""
    G, _, F = shape_a(C)
    if family == "exact":
        made = [[exact(C, 100000 + 100 * C + 10 * g + f) for f in range(F)] for g in range(G)]
        mats = np.array([[m.A for m in row] for row in made])
        vals = np.array([[m.values for m in row] for row in made])
        vals.setflags(write=False)
    else:
        mats = np.array([[free(C, 2 * C, 200000 + 100 * C + 10 * g + f) for f in range(F)] for g in range(G)])
        vals = None
    mats.setflags(write=False)
    return mats, vals


def ranks_a(C):
    """max_rank of (a): 1, 2, min(C, 5), C - 2, C - 1, C, clipped to 1 ... C"""
    return sorted({min(max(k, 1), C) for k in (1, 2, min(C, 5), C - 2, C - 1, C)})
