"""Reference for the value kernels of canonical coherence and of the imaginary interaction (sc_canonical_coherence_f64 and
sc_imaginary_interaction_f64, csrc/sc_canonical.hip) on records built by hand: joint cross-spectral matrices of channel groups whose
canonical coherences are known without rounding, Wishart matrices with a truth in extended precision, and the check of a returned
value in units of 2^-52.  NumPy only.

    exact(na, nb, coherences, seed)   the joint matrix of a pair with the given canonical coherences (``exact_groups``: any number of groups)
    free(sizes, n_obs, seed)          X^H X / n_obs of complex Gaussian coefficients with unequal channel gains, groups interleaved
    truth_free(S, a, b, view)         rho_1 by the generalised Rayleigh quotient in np.longdouble, MIM by a refined solve
    numpy_values(S, a, b, view)       the plain float64 reference: numpy.linalg.cholesky, two triangular solves, svd
    check(kind, got, truth, ...)      |got - truth| in units of 2^-52 (MIM: 2^-52 min(na, nb); conditioning series: x (kappa_a + kappa_b))

Two read views of a record (csrc/sc_canonical.hip): "canonical" takes S as it stands, M = L_a^-1 S_ab L_b^-H with S_gg = L_g L_g^H, and
returns rho_1^2 = lambda_max(M M^H); "interaction" takes Re S_gg and Im S_ab, M = L_a^-1 Im S_ab L_b^-T with Re S_gg = L_g L_g^T, and
returns MIC = rho_1 and MIM = trace(M M^T) = sum rho_k^2.

The ``exact`` family.  A mixer of n channels is W = (block-diagonal over the powers of two m of the binary expansion of n of
D H_m 2^-floor(log2(m) / 2)) x diag(gains): H_m the +-1 Hadamard matrix, D a random diagonal of powers of i (of signs in the
interaction view, where W is real), gains in {1, 2}.  H_m / sqrt(m) is unitary, so W W^H has the eigenvalues gain^2 x (1 or 2) and
cond(S_gg) <= 8.  With S_aa = W_a W_a^H, S_bb = W_b W_b^H and S_ab = W_a [diag(rho) | 0] W_b^H (i W_a [diag(rho) | 0] W_b^T in the
interaction view) every entry is a short dyadic number, and ANY Cholesky whitening gives M = Q_a [diag(rho) | 0] Q_b^H with Q_g =
L_g^-1 W_g unitary: dense inside the blocks, singular values exactly rho.  The products are formed in np.longdouble and the builder
asserts that float64 holds every entry.  The channels of the groups are interleaved over the C signals by one random permutation,
and a group's member list is in that (shuffled) order.

The bars K_CANONICAL, K_MIC, K_MIM and K_CONDITIONING are 8 x the worst ratio ``numpy_values`` reaches over the cases of (a) of
tests/test_gpu_canonical_values.py (the conditioning series for the last), rounded up to a power of two:
tools/canonical_values_accuracy.py --cpu prints them (profiles/canonical_values_accuracy.txt).  No device number enters them.
"""
import functools
from types import SimpleNamespace

import numpy as np

import epilogue_ref as eref
import global_coherence_ref as gref
from global_coherence_ref import blocks_of, hadamard, record       # noqa: F401  (the device tests take them from here)

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52
N_OBS = 8                                                           # of the records: a power of two, the division is exact

# tools/canonical_values_accuracy.py --cpu, the two ``max`` lines and the last one (profiles/canonical_values_accuracy.txt):
#                max     12.50      9.00      1.00
#                max     0.018
#   K = 8 x the NumPy maximum, rounded up to a power of two: canonical 128, MIC 128, MIM 8, conditioning 1
K_CANONICAL, K_MIC, K_MIM = 128.0, 128.0, 8.0
K_CONDITIONING = 1.0
BARS = {"canonical": K_CANONICAL, "mic": K_MIC, "mim": K_MIM}

# (a): the edges of CB_C = 16, of the member strides 16 / 32 / 128, of CBH_SMALL = 64, CBH_LDS_N = 96 and CBIG_C = 128
PAIR_SIZES = ((1, 1), (1, 2), (2, 2), (3, 5), (15, 16), (16, 16),
              (1, 17), (16, 17), (17, 17), (31, 32), (32, 33),
              (63, 64), (64, 64), (1, 65), (64, 65), (65, 65),
              (95, 96), (96, 96), (96, 97), (97, 97), (97, 128), (127, 128), (128, 128))
FAMILIES = ("exact", "free")
VIEWS = ("canonical", "interaction")
BINS_A = 2                                                          # bins of a record of (a), a different matrix in each
CONDITIONING = (10, 20, 30)                                         # p of the conditioning series: gains 2^0 ... 2^(p / 2)
CONDITIONING_SIZES = ((16, 16), (64, 64), (128, 128))

# The Jacobi kernels (SC_CANON_EIG=jacobi) stop a sweep early when off <= tol dia, off the sum of |b_pq|^2 above the diagonal and dia
# the sum of b_pp^2 (canonical_pair_kernel: tol = jtol = 1e-24 up to 16 channels; canonical_kernel<32>: 1e-30 up to 32; gc_jacobi
# in csrc/sc_jacobi.h for canonical_big_kernel: 1e-28 beyond).  The diagonal then differs from the eigenvalues by at most the
# 2-norm of the Hermitian off-diagonal part E, ||E||_2 <= ||E||_F = sqrt(2 off) <= sqrt(2 tol) ||diag||_F, and ||diag||_F <= ||B||_F =
# sqrt(sum rho_k^4) <= sqrt(min(na, nb)) rho_1^2.  (Quadratic convergence usually ends far below that; the rule promises no more.)


def jacobi_tolerance(max_group):
    return 1e-24 if max_group <= 16 else (1e-30 if max_group <= 32 else 1e-28)


def jacobi_allowance(na, nb, max_group, value=1.0):
    """what the stopping rule allows on rho_1^2 (<= ``value``), in units of 2^-52"""
    return float(np.sqrt(2.0 * jacobi_tolerance(max_group) * min(na, nb)) * value / EPS)


# ---- the exact family --------------------------------------------------------------------------------------------------------------
_RE, _IM = np.array([1.0, 0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0, -1.0])   # i^k


def mixer(n, rng, real, gain_exponents):
    """W [n, n] complex128 of the module docstring; ``gain_exponents``: the gains are 2^e with e drawn from them (the first and the
    last of them occur when n >= 2)."""
    W = np.zeros((n, n), dtype=np.complex128)
    o = 0
    for m in blocks_of(n):
        k = rng.integers(0, 2, m) * 2 if real else rng.integers(0, 4, m)
        H = hadamard(m) * 2.0 ** -((m.bit_length() - 1) // 2)
        W[o:o + m, o:o + m] = eref.as_complex(H * _RE[k][:, None], H * _IM[k][:, None])
        o += m
    e = rng.choice(np.asarray(gain_exponents), size=n)
    if n >= 2:
        where = rng.permutation(n)
        e[where[0]], e[where[1]] = gain_exponents[0], gain_exponents[-1]
    return W * 2.0 ** e.astype(np.float64)[None, :]


def _exactly(Z, what):
    """the complex128 matrix equal to the np.clongdouble matrix Z; asserts that no entry is rounded"""
    out = eref.as_complex(Z.real.astype(np.float64), Z.imag.astype(np.float64)) + 0.0
    assert np.array_equal(out.real.astype(LD), Z.real) and np.array_equal(out.imag.astype(LD), Z.imag), f"{what}: float64 does not hold an entry"
    return out


def exact_groups(sizes, rhos, seed, view="canonical", gain_exponents=(0, 1), max_cond=16.0, free_part=True):
    """The joint matrix of len(sizes) groups.  ``rhos``: {(a, b): coherences} for the pairs a < b that are coupled (at most min(n_a,
    n_b) numbers in 0 ... 1 each, in any order; a pair left out has a zero cross block).  view = "interaction": real mixers, the
    coherences sit in the IMAGINARY part of the cross blocks, and (``free_part``) the parts that view must not read -- the real part
    of the cross blocks, the imaginary part of the group blocks -- hold arbitrary dyadic numbers.
    Returns S [C, C] complex128 (exactly Hermitian), ``groups`` (the member list of every group, shuffled), ``rho`` {(a, b): the
    coherences as given, float64}, ``kappa`` [G] (cond of every group block as the view reads it) and ``mixers``."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no extended precision here: no reference"
    rng = np.random.default_rng(seed)
    G, C = len(sizes), int(sum(sizes))
    real = view == "interaction"
    W = [mixer(n, rng, real, gain_exponents) for n in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)])
    Z = np.zeros((C, C), dtype=CLD)
    kappa = np.zeros(G)
    for g in range(G):
        s = slice(off[g], off[g + 1])
        Z[s, s] = W[g].astype(CLD) @ W[g].astype(CLD).conj().T
        kappa[g] = np.linalg.cond(_exactly(Z[s, s], "group block"))
        assert max_cond is None or kappa[g] <= max_cond, (sizes, g, kappa[g])
    rho = {}
    for (a, b), r in rhos.items():
        assert 0 <= a < b < G
        r = np.asarray(r, dtype=np.float64)
        assert r.ndim == 1 and r.size <= min(sizes[a], sizes[b]) and (r >= 0).all() and (r <= 1).all()
        X = (W[a][:, :r.size].astype(CLD) * r.astype(LD)) @ W[b][:, :r.size].astype(CLD).conj().T
        if real:
            X = X * CLD(1j)
        sa, sb = slice(off[a], off[a + 1]), slice(off[b], off[b + 1])
        Z[sa, sb], Z[sb, sa] = X, X.conj().T
        rho[(a, b)] = r
    if real and free_part:
        for a in range(G):
            for b in range(a, G):
                sa, sb = slice(off[a], off[a + 1]), slice(off[b], off[b + 1])
                R = rng.integers(-64, 65, (sizes[a], sizes[b])).astype(LD) / 64
                if a == b:
                    R = R - R.T                                     # the imaginary part of a group block is antisymmetric
                    Z[sa, sa] = Z[sa, sa] + CLD(1j) * R
                else:
                    Z[sa, sb], Z[sb, sa] = Z[sa, sb] + R, Z[sb, sa] + R.T
    S = _exactly(Z, "joint matrix")
    assert np.array_equal(S, S.conj().T)
    perm = rng.permutation(C)
    full = np.zeros((C, C), dtype=np.complex128)
    full[np.ix_(perm, perm)] = S
    groups = [perm[off[g]:off[g + 1]].astype(np.int64) for g in range(G)]
    return SimpleNamespace(S=full, groups=groups, rho=rho, kappa=kappa, mixers=W, view=view)


def exact(na, nb, coherences, seed, view="canonical", **kw):
    """The joint matrix of ONE pair of groups of na and nb channels with the given canonical coherences (``exact_groups``)."""
    return exact_groups((na, nb), {(0, 1): coherences}, seed, view, **kw)


def distinct_coherences(n, seed):
    """n different multiples of 2^-10 in 2^-10 ... 1 - 2^-10"""
    return np.random.default_rng(seed).choice(np.arange(1, 1024), size=n, replace=False) / 1024.0


def truth_exact(rho):
    """{canonical: rho_1^2, mic: rho_1, mim: sum rho_k^2} in np.longdouble for the coherences of a pair"""
    r = np.asarray(rho, dtype=np.float64).astype(LD)
    if r.size == 0:
        r = np.zeros(1, dtype=LD)
    return {"canonical": r.max() ** 2, "mic": r.max(), "mim": (np.sort(r) ** 2).sum()}


# spectra of (d); n = min(na, nb) coherences each
def cluster(n, p, center=0.75):
    """center + k 2^-p, k = 0 ... n - 1"""
    return center + np.arange(n) * 2.0 ** -p


def graded(n):
    """2^0 ... 2^-20 in n steps of whole powers of two (n >= 2)"""
    return 2.0 ** -np.round(np.linspace(0.0, 20.0, n)) if n > 1 else np.ones(1)


SPECTRA = {
    "all_equal": lambda n: np.full(n, 0.625),
    "rho_1_is_one": lambda n: np.r_[1.0, distinct_coherences(n, 31)[:n - 1] * 0.75],
    "top_two_equal": lambda n: np.r_[0.875, 0.875, distinct_coherences(n, 32)[:max(n - 2, 0)] * 0.75][:n],
    "single_non_zero": lambda n: np.r_[0.8125, np.zeros(n - 1)],
    "all_zero": lambda n: np.zeros(n),
    "graded": graded,
}
CLUSTER_P = (20, 30, 36, 40, 44, 48)
# The entries of the cross block are sums of +- gain_a gain_b rho_k over a Hadamard block: with gains in {1, 2} they reach 0.75 x 4 m
# on a grid of 2^-p, so float64 holds them up to p = 40 at m = 128.  Beyond, the gains are all 1: the entries off the diagonal of a
# block are then 2^-p sum +- k (the 0.75 cancel between orthogonal rows), those on it 0.75 m + 2^-p m (m - 1) / 2 -- at most p + 2 bits.
CLUSTER_UNIT_GAINS_FROM = 44


def cluster_case(n, p, seed, view):
    return exact(n, n, cluster(n, p), seed, view, gain_exponents=(0, 1) if p < CLUSTER_UNIT_GAINS_FROM else (0, 0))


# ---- the free family ---------------------------------------------------------------------------------------------------------------
def free(sizes, n_obs, seed):
    """X^H X / n_obs of complex Gaussian coefficients with channel gains 2^-2 ... 2^2 (gref.free) for sum(sizes) signals; the groups
    are interleaved by one random permutation and listed in shuffled order.  Returns S and ``groups``."""
    C = int(sum(sizes))
    S = gref.free(C, n_obs, seed)
    perm = np.random.default_rng(seed + 1).permutation(C)
    off = np.concatenate([[0], np.cumsum(sizes)])
    return SimpleNamespace(S=S, groups=[perm[off[g]:off[g + 1]].astype(np.int64) for g in range(len(sizes))], view=None)


def blocks(S, a, b, view):
    """(S_aa, S_bb, S_ab) as the view reads them: complex, or (Re, Re, Im) as real float64"""
    a, b = np.asarray(a), np.asarray(b)
    Saa, Sbb, Sab = S[np.ix_(a, a)], S[np.ix_(b, b)], S[np.ix_(a, b)]
    if view == "interaction":
        return np.ascontiguousarray(Saa.real), np.ascontiguousarray(Sbb.real), np.ascontiguousarray(Sab.imag)
    return Saa, Sbb, Sab


def numpy_pair(Saa, Sbb, Sab):
    """The plain float64 reference: (singular values of M = L_a^-1 S_ab L_b^-H, largest first; filters alpha = L_a^-H u_1 and
    beta = L_b^-H v_1) by numpy.linalg.cholesky, two triangular solves and svd."""
    La, Lb = np.linalg.cholesky(Saa), np.linalg.cholesky(Sbb)
    M = np.linalg.solve(Lb, np.linalg.solve(La, Sab).conj().T).conj().T
    U, sv, Vh = np.linalg.svd(M)
    alpha, beta = np.linalg.solve(La.conj().T, U[:, 0]), np.linalg.solve(Lb.conj().T, Vh[0].conj())
    return sv, alpha, beta


def numpy_values(S, a, b, view):
    """{canonical: rho_1^2} or {mic: rho_1, mim: sum rho_k^2} of the plain float64 reference"""
    sv = numpy_pair(*blocks(S, a, b, view))[0]
    return {"canonical": sv[0] ** 2} if view == "canonical" else {"mic": sv[0], "mim": float((sv ** 2).sum())}


def _form_ld(x, A, y):
    """(re, im) of x^H A y in np.longdouble"""
    re, im = gref.cmatmul_ld(np.conj(x)[None, :], A)                # [1, n] each
    yr, yi = np.asarray(y).real.astype(LD), np.asarray(y).imag.astype(LD)
    return (re[0] * yr - im[0] * yi).sum(), (re[0] * yi + im[0] * yr).sum()


def _split(X):
    hi = X.astype(np.float64)
    return hi, (X - hi.astype(LD)).astype(np.float64)


def _solve_refined(R, B):
    """R^-1 B in np.longdouble for real float64 R (symmetric positive definite) and B: a float64 solve refined twice with residuals in
    extended precision"""
    X = np.linalg.solve(R, B).astype(LD)
    for _ in range(2):
        hi, lo = _split(X)
        resid = B.astype(LD) - gref.matmul_ld(R, hi) - gref.matmul_ld(R, lo)
        X = X + np.linalg.solve(R, resid.astype(np.float64)).astype(LD)
    return X


def truth_free(S, a, b, view, max_estimate=2.0 ** -60):
    """The truth of a pair of a ``free`` matrix, np.longdouble.  rho_1 is the generalised Rayleigh quotient |alpha^H S_ab beta| /
    sqrt((alpha^H S_aa alpha)(beta^H S_bb beta)) at the float64 filters of ``numpy_pair``: stationary at the true filters, so its error
    is the square of theirs, estimated from the float64 spectrum as (2^-52 (kappa_a + kappa_b) / (rho_1^2 - rho_2^2))^2 and asserted
    to be below ``max_estimate``.  view = "interaction": MIM = trace(R_a^-1 I R_b^-1 I^T) from refined solves as well."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no extended precision here: no reference"
    Saa, Sbb, Sab = blocks(S, a, b, view)
    sv, alpha, beta = numpy_pair(Saa, Sbb, Sab)
    gap = sv[0] ** 2 - (sv[1] ** 2 if sv.size > 1 else 0.0)
    estimate = (EPS * (np.linalg.cond(Saa) + np.linalg.cond(Sbb)) / gap) ** 2
    assert estimate < max_estimate, (len(a), len(b), view, estimate)
    num = _form_ld(alpha, Sab, beta)
    rho1 = np.sqrt(num[0] ** 2 + num[1] ** 2) / np.sqrt(_form_ld(alpha, Saa, alpha)[0] * _form_ld(beta, Sbb, beta)[0])
    if view == "canonical":
        return {"canonical": rho1 ** 2}
    X, Y = _solve_refined(Saa, Sab), _solve_refined(Sbb, Sab.T.copy())
    return {"mic": rho1, "mim": (X * Y.T).sum()}


# ---- the check ---------------------------------------------------------------------------------------------------------------------
def check(kind, got, truth, n_min=1, kappa=1.0):
    """The error of a returned value in units of 2^-52 (the outputs are at most 1): kind "canonical" (rho_1^2), "mic" (rho_1) or "mim"
    (sum rho_k^2, unit 2^-52 min(na, nb): pass ``n_min``).  ``kappa``: kappa_a + kappa_b for the conditioning series."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no extended precision here: no reference"
    assert kind in BARS
    got = np.float64(got)
    assert np.isfinite(got), f"{kind}: {got!r}"
    unit = LD(EPS) * (n_min if kind == "mim" else 1) * LD(kappa)
    return float(abs(LD(got) - LD(truth)) / unit)


# ---- the cases of (a) --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_a(family, sizes, view):
    """(mats [BINS_A, C, C], groups, truths [BINS_A] of {kind: np.longdouble}) of a case of (a); ``free`` has one record for both
    views (view picks the truth), ``exact`` one per view.  The member lists are those of bin 0's permutation in every bin."""
    na, nb = sizes
    made, truths = [], []
    for f in range(BINS_A):
        seed = 1000 * na + 10 * nb + f
        if family == "exact":
            m = exact(na, nb, distinct_coherences(min(na, nb), seed + 5), seed, view)
            t = truth_exact(m.rho[(0, 1)])
            t = {"canonical": t["canonical"]} if view == "canonical" else {"mic": t["mic"], "mim": t["mim"]}
        else:
            m = free(sizes, 2 * (na + nb), seed)
        made.append(m)
        truths.append(t if family == "exact" else None)
    groups = made[0].groups
    mats = np.array([_as_grouped(m, groups) for m in made])
    if family == "free":
        truths = [truth_free(mats[f], groups[0], groups[1], view) for f in range(BINS_A)]
    mats.setflags(write=False)
    return mats, groups, truths


def _as_grouped(m, groups):
    """the matrix of m with its groups moved onto the member lists ``groups`` (same sizes)"""
    C = m.S.shape[0]
    src, dst = np.concatenate(m.groups), np.concatenate(groups)
    out = np.zeros((C, C), dtype=np.complex128)
    out[np.ix_(dst, dst)] = m.S[np.ix_(src, src)]
    return out


def stack_bins(made):
    """(mats [F, C, C], groups) of several ``exact`` / ``free`` results with the same group sizes: every bin on the member lists of the first"""
    return np.array([_as_grouped(m, made[0].groups) for m in made]), made[0].groups


@functools.lru_cache(maxsize=None)
def conditioning_case(sizes, p, view):
    """family ``exact`` with gains 2^0 ... 2^(p / 2): (matrix, groups, truth, kappa_a + kappa_b)"""
    na, nb = sizes
    seed = 7000 + 10 * na + p
    m = exact(na, nb, distinct_coherences(min(na, nb), seed), seed, view, gain_exponents=tuple(range(p // 2 + 1)), max_cond=None)
    return m.S, m.groups, truth_exact(m.rho[(0, 1)]), float(m.kappa.sum())


def numpy_ratios(family, sizes):
    """the worst ratios {kind: ratio} of ``numpy_values`` over the bins of a case of (a)"""
    worst = {}
    for view in VIEWS:
        mats, groups, truths = case_a(family, sizes, view)
        for f in range(mats.shape[0]):
            got = numpy_values(mats[f], groups[0], groups[1], view)
            for kind, v in got.items():
                worst[kind] = max(worst.get(kind, 0.0), check(kind, v, truths[f][kind], min(sizes)))
    return worst


def numpy_conditioning_ratio(sizes, p):
    """the worst ratio of ``numpy_values`` on a case of the conditioning series, all three kinds, unit 2^-52 (kappa_a + kappa_b)"""
    worst = 0.0
    for view in VIEWS:
        S, groups, truth, kappa = conditioning_case(sizes, p, view)
        for kind, v in numpy_values(S, groups[0], groups[1], view).items():
            worst = max(worst, check(kind, v, truth[kind], min(sizes), kappa))
    return worst


def bar_from(worst):
    """8 x the worst NumPy ratio, rounded up to a power of two (at least 1)"""
    k = 1.0
    while k < 8.0 * worst:
        k *= 2.0
    return k
