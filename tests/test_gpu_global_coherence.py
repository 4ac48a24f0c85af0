"""The global-coherence eigensolvers (sc_global_coherence_f64, csrc/sc_global.hip) on records built by hand: no stage A, no stage B,
no Multitaper.  tests/global_coherence_ref.py builds Hermitian matrices whose eigenpairs are known without rounding (``exact``),
Wishart matrices (``free``) and the structures that steer the Householder kernel into its branches, packs n_obs x matrix into a
record with SC_PLANE_CSM, and measures a result in extended precision: values, eigen-residual, Gram matrix and phase, in units of
2^-52 ||A||_2 (2^-52 for the last two).  The bars are 8 x what numpy.linalg.eigh reaches on the cases of (a), rounded up to a power
of two (profiles/global_coherence_accuracy.txt); no device number enters them.  The kernel is chosen by the signal count:

  1 ... 32     global_coherence_kernel: cyclic Jacobi, matrix and vectors in LDS (dummy player and alignment arithmetic at odd counts)
  33 ... 256   global_coherence_eigh_kernel<256>: Householder, bisection, inverse iteration, a wave per vector back-transformed
  257 ... 512  global_coherence_eigh_kernel<512>: eight elements of every vector per lane
  SC_GLOBAL_EIG=jacobi: the LDS kernel up to 64, global_coherence_big_kernel<512> (<256> with SC_GLOBAL_NT256) up to 128, <1024> up to 256

(a) every tier at its edges, both families, max_rank 1, 2, 5, C - 2, C - 1, C, both orders: all four ratios under their bars.
(b) the record: F = N / 2 + 1 against F = N, permuted windows, float records, n_obs = 12, two runs.
(c) the persistent loop takes a second item (more bins than slots): identity reflections followed by dense matrices and the reverse.
(d) structure: dead channel, tridiagonal, imaginary sub-diagonal, c I, 1 1^T, two identical blocks, multiplicity 16, graded spectrum.
(e) fewer observations than signals: a cluster of zero eigenvalues next to the last one asked for.
(f) tesla^2 and count^2 amplitudes.
(g) the diagnostic kernels against their own stopping rule and against the default kernel.
(h) nothing is stored outside ``values`` and ``vectors``, and all of both is written.
(i) the argument checks return their codes and write nothing.

What the suite found when it first ran (fixed in csrc/sc_global.hip and csrc/sc_jacobi.h): Gram ratios of 358 ... 425
in (a) at 34, 64 and 127 signals (vectors just outside a cluster of the inverse iteration), a dead channel's eigenvalue of 1e-35
instead of 0 in (d) (by the arithmetic of the bisection: fixed before the case ran), and in (g) residuals of 1e-8 ||A|| from
global_coherence_big_kernel<256 / 512> (the convergence test of gc_jacobi cancelled) and values / Gram of 264 / 270 from <1024> at 256 signals.

What each part is there to catch -- expectations from reading the kernel, not mutations that were run:
  the bisection loop cut to 30 iterations (values 2^-30 ||T|| wide instead of 2^-52): the value ratio of (a) from 33 signals on;
  the barrier at the top of the item loop removed, or tau[k] not reset in the H = I branch (a stale reflector of the previous item is
  applied in the back-transformation): the residual of (c), and of (d) where a dense bin precedes a diagonal one in one launch;
  the ``i < C`` guard of the back-transformation dropped (columns read and vectors stored past C): the bands of (h), the residual
  of (a) at 257 and 300 signals.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as eref                                                   # noqa: E402
import global_coherence_ref as gref                                           # noqa: E402
from guarded_buffers import BAND, FILL, guarded, guarded_memory, intact       # noqa: E402
from spectral_connectivity_amd import _lib, _stage_d, engine                  # noqa: E402

# tools/global_coherence_accuracy.py --cpu (profiles/global_coherence_accuracy.txt):
#             max     27.49     18.29     17.06      0.29
#   K = 8 x the NumPy maximum, rounded up to a power of two: values 256, residual 256, Gram 256
K_VALUES, K_RESIDUAL, K_GRAM, K_PHASE = gref.K_VALUES, gref.K_RESIDUAL, gref.K_GRAM, gref.K_PHASE
assert (K_VALUES, K_RESIDUAL, K_GRAM) == (256.0, 256.0, 256.0)
SC_EINVAL, SC_EUNSUPPORTED = -1, -5
CSM = eref.PLANE_CSM
N_OBS = gref.N_OBS


def upload(rec):
    _lib.require_gpu()
    return torch.from_numpy(np.ascontiguousarray(rec)).to("cuda:0")


def run(accum, G, F, N, C, n_obs, max_rank, ascending):
    """(values [G, N, K], vectors [G, N, C, K]) of the records ``accum`` on the device, as NumPy arrays"""
    values, vectors = engine.global_coherence(accum, G, F, N, C, CSM, n_obs, max_rank, ascending)
    assert tuple(values.shape) == (G, N, max_rank) and values.dtype == torch.float64
    assert tuple(vectors.shape) == (G, N, C, max_rank) and vectors.dtype == torch.complex128
    return values.cpu().numpy(), vectors.cpu().numpy()


def solve(mats, max_rank, ascending, n_obs=N_OBS, dtype=np.float64, two_sided=True):
    """(values, vectors, stack) of ``mats`` [G, F, C, C] packed by gref.record"""
    G, F, C, _ = mats.shape
    rec, stack = gref.record(mats, n_obs, dtype, two_sided)
    values, vectors = run(upload(rec), G, F, stack.shape[1], C, n_obs, max_rank, ascending)
    return values, vectors, stack


def jacobi_bars(A):
    """The bars of a Jacobi kernel for the matrix A: the residual bar is the larger of K_RESIDUAL 2^-52 ||A||_2 and 2e-14 ||A||_F
    (gref.JACOBI_RESIDUAL: the kernels stop at off^2 <= 1e-28 dia^2)."""
    ratio = gref.JACOBI_RESIDUAL * np.linalg.norm(A) / (gref.EPS * np.linalg.norm(A, 2))
    return dict(gref.BARS, residual=max(K_RESIDUAL, float(ratio)))


def check_bins(stack, values, vectors, ascending, exact_values=None, what="", jacobi=None, bars=None):
    """Every (group, bin) of a result against its matrix of the two-sided ``stack``: the worst ratios, all under their bars.
    ``exact_values`` [G, N, C]; ``jacobi``: the bars of the Jacobi kernels (default: by the signal count)."""
    C = stack.shape[-1]
    jacobi = C <= 32 if jacobi is None else jacobi
    worst, bad = {}, []
    for g in range(stack.shape[0]):
        for n in range(stack.shape[1]):
            r = gref.check(stack[g, n], values[g, n], vectors[g, n], ascending, None if exact_values is None else exact_values[g, n])
            b = bars or (jacobi_bars(stack[g, n]) if jacobi else gref.BARS)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
            bad += [(g, n, k, v, b[k]) for k, v in gref.over_the_bars(r, b).items()]
    print(f"\n  {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not bad, (what, bad)
    return worst


def two_sided_values(vals, N):
    """exact values [G, F, C] of the accumulated bins -> [G, N, C] of the two-sided ones (a conjugate has the same eigenvalues)"""
    return None if vals is None else np.stack([vals[:, n if n < vals.shape[1] else N - n] for n in range(N)], axis=1)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- (a) every tier at its edges ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def record_a(family, C):
    """(device record, two-sided stack, exact values per two-sided bin or None) of a case of (a): uploaded once per case"""
    mats, vals = gref.cases_a(family, C)
    G, N, F = gref.shape_a(C)
    rec, stack = gref.record(mats, N_OBS, np.float64, F == N)
    assert np.array_equal(stack[:, :F], mats)
    stack.setflags(write=False)
    return upload(rec), stack, two_sided_values(vals, N)


def device_result(family, C, max_rank, ascending):
    G, N, F = gref.shape_a(C)
    accum, stack, vals = record_a(family, C)
    values, vectors = run(accum, G, F, N, C, N_OBS, max_rank, ascending)
    return stack, values, vectors, vals


def bars_of(family, C):
    """the bars of a case of (a) (the Jacobi kernel's residual bar depends on the matrix: the largest of the case)"""
    if C > 32:
        return gref.BARS
    stack = record_a(family, C)[1]
    return dict(gref.BARS, residual=max(jacobi_bars(A)["residual"] for A in stack.reshape(-1, C, C)))


def device_ratios(family, C, max_rank, ascending):
    """the worst ratios of a case of (a) (tools/global_coherence_accuracy.py)"""
    stack, values, vectors, vals = device_result(family, C, max_rank, ascending)
    worst = {}
    for g in range(stack.shape[0]):
        for n in range(stack.shape[1]):
            r = gref.check(stack[g, n], values[g, n], vectors[g, n], ascending, None if vals is None else vals[g, n])
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    return worst


CASES_A = [(family, C, K, asc) for C in gref.SIZES for family in gref.FAMILIES for K in gref.ranks_a(C) for asc in (False, True)]


@pytest.mark.parametrize("family,C,max_rank,ascending", CASES_A)
def test_every_tier_at_its_edges(family, C, max_rank, ascending):
    stack, values, vectors, vals = device_result(family, C, max_rank, ascending)
    check_bins(stack, values, vectors, ascending, vals, f"{family} C = {C} max_rank = {max_rank} ascending = {ascending}")


# ---- (b) record plumbing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,max_rank", [(5, 5), (40, 40), (130, 4), (260, 3)])
def test_half_records_against_full_records(C, max_rank):
    """F = N / 2 + 1 = 3 accumulated bins against F = N = 4 holding the same four matrices: the values are equal, and the vectors of
    bin 3 are the conjugates of those of bin 1 within the Gram bar (entries of unit vectors, 2^-52 each)."""
    mats = np.array([[gref.exact(C, 300 + 10 * g + f).A for f in range(3)] for g in range(2)])
    v_half, x_half, stack = solve(mats, max_rank, False, two_sided=False)
    assert stack.shape[1] == 4 and np.array_equal(stack[:, 3], mats[:, 1].conj())
    v_full, x_full, stack_full = solve(stack, max_rank, False, two_sided=True)
    assert np.array_equal(stack_full, stack)
    assert np.array_equal(v_half, v_full), "values differ between F = N / 2 + 1 and F = N"
    assert np.array_equal(v_half[:, 3], v_half[:, 1]), "a conjugated bin has other values"
    for x in (x_half, x_full):
        assert np.abs(x[:, 3] - x[:, 1].conj()).max() <= K_GRAM * gref.EPS
    assert np.abs(x_half - x_full).max() <= K_GRAM * gref.EPS
    check_bins(stack, v_half, x_half, False, what=f"half records C = {C}")


@pytest.mark.parametrize("C,max_rank", [(17, 17), (65, 65), (260, 3)])
def test_windows_float_records_and_repeated_runs(C, max_rank):
    """Permuting the windows permutes the outputs, float records of the ``exact`` family give the bits of double records, and two
    runs give the same bits."""
    mats = np.array([[gref.exact(C, 500 + 10 * g + f).A for f in range(3)] for g in range(3)])
    v, x, _ = solve(mats, max_rank, True, two_sided=False)
    again = solve(mats, max_rank, True, two_sided=False)
    assert same_bits(v, again[0]) and same_bits(x, again[1]), "two runs differ"
    perm = [2, 0, 1]
    moved = solve(mats[perm], max_rank, True, two_sided=False)
    assert same_bits(v[perm], moved[0]) and same_bits(x[perm], moved[1]), "a window's result depends on its neighbours"
    floats = solve(mats, max_rank, True, dtype=np.float32, two_sided=False)
    assert same_bits(v, floats[0]) and same_bits(x, floats[1]), "float records differ from double records holding the same numbers"


@pytest.mark.parametrize("C", [12, 70])
def test_twelve_observations(C):
    """n_obs = 12: the division inside the kernel rounds, and the matrix it must decompose is the rounded one"""
    mats = np.array([[gref.free(C, 12, 700 + 10 * g + f) for f in range(3)] for g in range(2)])
    for ascending in (False, True):
        v, x, stack = solve(mats, min(C, 12), ascending, n_obs=12, two_sided=False)
        check_bins(stack, v, x, ascending, what=f"n_obs = 12, C = {C}")


# ---- (c) the persistent loop -------------------------------------------------------------------------------------------------------
def eigh_slots(bins, C, max_rank):
    """The workgroups sc_global_coherence_f64 launches beyond 32 signals, from its code: per_slot = C^2 complex128 (the matrix) +
    8 C max_rank doubles (the work arrays); slots = min(bins, 1024, 1 GB / per_slot), at least 1."""
    per_slot = C * C * 16 + 8 * C * max_rank * 8
    return max(1, min(bins, 1024, (1 << 30) // per_slot))


@pytest.mark.parametrize("C,max_rank,G,N,dense", [(33, 1, 129, 8, "free"), (512, 512, 28, 2, "exact")])
def test_a_workgroup_takes_a_second_item(C, max_rank, G, N, dense):
    """More bins than slots: workgroup b decomposes item b and then item b + slots, on the same tau, d, e, matrix scratch and work
    arrays.  Items 0 and 1 are dense, the rest of the first pass is diagonal (every tau = 0); the successors of the dense items are
    diagonal (a stale reflector would be applied to them) and the other items of the second pass are dense (a tau left at 0 would
    skip their reflections).  Two matrices of each kind: each is checked once, and every bin that repeats it must repeat its bits."""
    bins = G * N
    slots = eigh_slots(bins, C, max_rank)
    assert slots + 4 <= bins <= 2 * slots, (bins, slots)          # the formula above changed: this test would run one pass only
    assert slots == {33: 1024, 512: 51}[C]
    if dense == "free":
        full = [gref.free(C, 2 * C, 900 + k) for k in range(2)]
        exact_values = [None, None]
    else:
        made = [gref.exact(C, 900 + k) for k in range(2)]
        full, exact_values = [m.A for m in made], [m.values for m in made]
    diag = [np.diag((np.arange(C) * 7 % C + 1.0 + k) / 4.0).astype(np.complex128) for k in range(2)]
    unique = np.array(full + diag)[None]                          # [1, 4, C, C]: 0, 1 dense; 2, 3 diagonal
    kind = np.empty(bins, dtype=int)
    for item in range(bins):
        first = item % slots
        is_dense = (first < 2) == (item < slots)
        kind[item] = (0 if is_dense else 2) + (item + item // slots) % 2
    assert set(kind[:2]) == {0, 1} and set(kind[2:slots]) == {2, 3} and set(kind[slots:slots + 2]) == {2, 3} and set(kind[slots + 2:]) == {0, 1}
    rec_u, stack_u = gref.record(unique, N_OBS, np.float32 if dense == "exact" else np.float64, True)
    values, vectors = run(upload(rec_u[kind]), G, N, N, C, N_OBS, max_rank, False)
    values, vectors = values.reshape(bins, max_rank), vectors.reshape(bins, C, max_rank)
    for k in range(4):
        where = np.flatnonzero(kind == k)
        assert (where < slots).any() and (where >= slots).any()
        first = where[0]
        for item in where[1:]:
            assert same_bits(values[item], values[first]) and same_bits(vectors[item], vectors[first]), \
                f"item {item} (pass {item // slots}) differs from item {first} holding the same matrix"
        ex = (exact_values + [np.diag(diag[0]).real, np.diag(diag[1]).real])[k]
        check_bins(stack_u[:, k:k + 1], values[first][None, None], vectors[first][None, None], False,
                   None if ex is None else ex[None, None], f"second item, C = {C}, matrix {k}")


# ---- (d) structure -----------------------------------------------------------------------------------------------------------------
def special_ranks(name, C):
    return {"scaled_identity": (C,), "two_blocks": (C,), "rank_one": (1, 2)}.get(name, (1, C))


@pytest.mark.parametrize("C", [6, 32, 40, 130, 260])
@pytest.mark.parametrize("name", list(gref.SPECIAL))
def test_special_matrices(name, C):
    """Each special matrix as bins 1 and 2 of one window behind a dense bin 0 (so that, where a workgroup would take several, the
    identity reflections follow real ones), bin 2 doubled.  c I and the two identical blocks with max_rank = C: the whole spectrum is
    one cluster, or C / 2 pairs.  The dead channel's eigenvalue is exactly 0."""
    A = gref.SPECIAL[name](C)
    mats = np.array([[gref.exact(C, 1100 + C).A, A, 2.0 * A]])
    for max_rank in special_ranks(name, C):
        v, x, stack = solve(mats, max_rank, False)
        check_bins(stack, v, x, False, what=f"{name} C = {C} max_rank = {max_rank}")
        assert np.array_equal(v[0, 2], 2.0 * v[0, 1]), "a matrix doubled does not double its values"
        if name == "dead_channel" and max_rank == C:
            assert v[0, 1, -1] == 0.0 and v[0, 2, -1] == 0.0, f"dead channel: eigenvalue {v[0, 1, -1]!r}, not 0"
        if name == "rank_one":
            assert abs(v[0, 1, 0] - C) <= K_VALUES * gref.EPS * C and (max_rank == 1 or v[0, 1, 1] <= K_VALUES * gref.EPS * C)


@pytest.mark.parametrize("ascending", [False, True])
def test_multiplicity_sixteen(ascending):
    """C = 64 with eigenvalues of multiplicity 2, 4 and 16: residual and Gram say the right thing, any orthonormal basis passes"""
    made = [gref.exact(64, 1300 + k, eigenvalues=gref.with_multiplicities(64, 1300 + k)) for k in range(3)]
    v, x, stack = solve(np.array([[m.A for m in made]]), 64, ascending, two_sided=False)
    vals = two_sided_values(np.array([[m.values for m in made]]), 4)
    check_bins(stack, v, x, ascending, vals, "multiplicities 2, 4, 16 at C = 64")


def test_graded_spectrum():
    """C = 48, eigenvalues 2^0 ... 2^-40: the bars are absolute in ||A|| = 1 (the small values are not expected to be relatively
    accurate); double records, float32 does not hold these entries."""
    made = [gref.exact(48, 1400 + k, eigenvalues=gref.graded(48)) for k in range(3)]
    for max_rank in (5, 48):
        v, x, stack = solve(np.array([[m.A for m in made]]), max_rank, False, two_sided=False)
        check_bins(stack, v, x, False, two_sided_values(np.array([[m.values for m in made]]), 4), f"graded spectrum, max_rank = {max_rank}")


# ---- (e) fewer observations than signals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,n_obs", [(20, 8), (40, 8), (100, 16), (300, 16)])
def test_fewer_observations_than_signals(C, n_obs):
    """X^H X of n_obs < C observations: C - n_obs eigenvalues are zero to rounding (bisection meets them as one cluster, some of them
    below zero and clamped), and max_rank = n_obs -- the largest the Python classes allow -- takes the last non-zero one next to it."""
    mats = np.array([[gref.free(C, n_obs, 1500 + C + f) for f in range(2)]])
    for max_rank in (1, n_obs):
        for ascending in (False, True):
            v, x, stack = solve(mats, max_rank, ascending, n_obs=n_obs)
            assert (v >= 0).all()
            check_bins(stack, v, x, ascending, what=f"C = {C}, {n_obs} observations, max_rank = {max_rank}")
            if max_rank == n_obs:
                last = v[..., 0] if ascending else v[..., -1]
                norm = v.max(axis=-1)
                assert (last > 1e-6 * norm).all(), f"the {n_obs}-th value is not separated from zero: {last / norm}"


# ---- (f) amplitude -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0 ** -90, 2.0 ** 44])
@pytest.mark.parametrize("C,max_rank", [(64, 64), (300, 6)])
def test_amplitudes_of_real_recordings(C, max_rank, scale):
    """tesla^2 (2^-90) and squares of 24-bit counts (2^44): float records, the same bars relative to the scaled ||A||; and the
    vectors are those of the unscaled run: eigenvectors of the unscaled matrix to the residual and Gram bars, each within the Gram
    bar of the unscaled run's in direction (<v, v'> = 1 to second order in their difference)."""
    made = [gref.exact(C, 1600 + C + f) for f in range(2)]
    unit = np.array([[m.A for m in made]])
    vals = np.array([[m.values for m in made]])
    v1, x1, stack1 = solve(unit, max_rank, False, dtype=np.float32)
    v, x, stack = solve(unit * scale, max_rank, False, dtype=np.float32)
    assert np.array_equal(stack, stack1 * scale)
    check_bins(stack, v, x, False, vals * scale, f"C = {C} x 2^{int(np.log2(scale))}")
    check_bins(stack1, v / scale, x, False, vals, f"C = {C} x 2^{int(np.log2(scale))}, vectors on the unscaled matrix")
    inner = np.einsum("gnck,gnck->gnk", x.conj(), x1)
    assert np.abs(inner - 1.0).max() <= K_GRAM * gref.EPS, np.abs(inner - 1.0).max() / gref.EPS


# ---- (g) the diagnostic kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,nt256", [(33, False), (64, False), (65, False), (128, False), (100, True), (129, False), (256, False)])
def test_diagnostic_jacobi_kernels(C, nt256, debug_env):
    """SC_GLOBAL_EIG=jacobi: the LDS kernel up to 64 signals, global_coherence_big_kernel<512> up to 128 (<256> with SC_GLOBAL_NT256),
    <1024> with the triangle in a global scratch up to 256.  All three stop when the off-diagonal mass of the rotated matrix is at
    most 1e-28 of the diagonal's (global_coherence_kernel: ``red[0][0] <= 1e-28 * red[1][0]`` over the full matrix; gc_jacobi the same
    over the entries above the diagonal, half the mass), so a column of A V - V diag(values) is at most sqrt(2) 1e-14 ||A||_F long:
    the residual bar is the larger of the ordinary one and 2e-14 ||A||_F (factor 2), the other bars are the ordinary ones.  The values
    equal the default kernel's within K_VALUES.  (max_rank = C up to 128 signals, in two or three batches of logged rotations.)"""
    big = C > 128
    G, F = (1, 2) if big else (2, 3)
    made = [[gref.exact(C, 1700 + C + 10 * g + f) for f in range(F)] for g in range(G)]
    mats = np.array([[m.A for m in row] for row in made])
    vals = np.array([[m.values for m in row] for row in made])
    max_rank = min(C, 5) if big else C
    v_default, _, stack = solve(mats, max_rank, False, two_sided=big)
    debug_env("SC_GLOBAL_EIG", "jacobi")
    if nt256:
        debug_env("SC_GLOBAL_NT256", "1")
    v, x, _ = solve(mats, max_rank, False, two_sided=big)
    check_bins(stack, v, x, False, two_sided_values(vals, stack.shape[1]), f"SC_GLOBAL_EIG=jacobi C = {C}", jacobi=True)
    norm = vals.max()
    assert np.abs(v - v_default).max() <= K_VALUES * gref.EPS * norm, np.abs(v - v_default).max() / (gref.EPS * norm)


def call(accum, G, F, N, C, planes, n_obs, max_rank, values, vectors):
    """the status of sc_global_coherence_f64 called through ctypes on raw buffers"""
    stream = engine.TorchMemory(torch.device("cuda:0")).stream()
    return _lib._handle().sc_global_coherence_f64(ctypes.c_void_p(accum.data_ptr()), G, F, N, C, planes, n_obs, max_rank, 0,
                                                  ctypes.c_void_p(values.data_ptr() + BAND), ctypes.c_void_p(vectors.data_ptr() + BAND), stream)


def refused(code, G, F, N, C, planes, n_obs, max_rank, alloc_C=None):
    """the call returns ``code`` and has written neither output"""
    _lib.require_gpu()
    cc = alloc_C or max(C, 1)
    lay = eref.layout(cc, CSM)
    accum = torch.zeros((G * F, lay.floats_per_bin), dtype=torch.float64, device="cuda:0")
    n_val, n_vec = G * N * cc * 8, G * N * cc * cc * 16
    values, vectors = guarded(n_val), guarded(n_vec)
    status = call(accum, G, F, N, C, planes | _lib.RECORD_F64, n_obs, max_rank, values, vectors)
    torch.cuda.synchronize()
    assert status == code, (status, _lib._handle().sc_last_error())
    for buf, n in ((values, n_val), (vectors, n_vec)):
        assert intact(buf, n) and bool((buf[BAND:BAND + n] == FILL).all()), "a refused call wrote"


def test_jacobi_switch_beyond_256_signals_is_refused(debug_env):
    debug_env("SC_GLOBAL_EIG", "jacobi")
    refused(SC_EUNSUPPORTED, 1, 2, 2, 257, CSM, 8, 1)


# ---- (h) bounds of the stores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 33, 130, 260])
def test_nothing_is_stored_outside_the_outputs(C):
    """``values`` and ``vectors`` between two 4 KB bands each: the bands survive, and every byte between them is written -- the
    outputs are the bits of the ordinary run, and no element is left at the fill pattern."""
    mats = np.array([[gref.exact(C, 1800 + C + f).A for f in range(2)]])
    rec, _ = gref.record(mats, N_OBS, np.float64, True)
    accum = upload(rec)
    fill = np.frombuffer(bytes([FILL]) * 8, dtype=np.float64)[0]
    for max_rank in (1, C):
        want = run(accum, 1, 2, 2, C, N_OBS, max_rank, False)
        mem = guarded_memory()
        values, vectors = _stage_d.global_coherence(mem, accum, 1, 2, 2, C, CSM, N_OBS, max_rank, False)
        torch.cuda.synchronize()
        assert mem.sizes() == [2 * max_rank * 8, 2 * C * max_rank * 16]
        assert mem.intact(), f"C = {C}, max_rank = {max_rank}: stored outside values or vectors"
        got = values.cpu().numpy(), vectors.cpu().numpy()
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        assert not (got[0] == fill).any() and not (got[1].real == fill).any() and not (got[1].imag == fill).any(), "an element was not written"


# ---- (i) argument checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,code,args", [
    ("max_rank = 0", SC_EINVAL, dict(max_rank=0)),
    ("max_rank = C + 1", SC_EINVAL, dict(max_rank=7)),
    ("C = 0", SC_EUNSUPPORTED, dict(C=0, alloc_C=6)),
    ("C = 513", SC_EUNSUPPORTED, dict(C=513, alloc_C=6)),
    ("n_obs = 0", SC_EINVAL, dict(n_obs=0)),
    ("F neither N nor N / 2 + 1", SC_EINVAL, dict(F=4, N=8)),
    ("F = N + 1", SC_EINVAL, dict(F=5, N=4)),
    ("no SC_PLANE_CSM", SC_EINVAL, dict(planes=eref.PLANE_UNIT)),
])
def test_argument_checks(what, code, args):
    """include/sc_hip.h: SC_EINVAL for a bad argument or shape, SC_EUNSUPPORTED for a signal count outside
    1 ... sc_global_coherence_max_signals(); either before anything is launched"""
    assert _lib._handle().sc_global_coherence_max_signals() == 512
    kw = dict(G=2, F=3, N=4, C=6, planes=CSM, n_obs=8, max_rank=2)
    kw.update(args)
    refused(code, **kw)
