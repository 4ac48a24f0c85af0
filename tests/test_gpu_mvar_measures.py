"""The MVAR measure kernels (sc_mvar_measure_f64, csrc/sc_mvar.hip) on factors built by hand: no stage A / B, no Wilson iteration,
so nothing hides behind that iteration's 1e-8.  tests/mvar_measures_ref.py builds G [P][N][C][C] and gives the eight quantities
(noise covariance, transfer function, MVAR coefficients, DTF, DC, PDC, gPDC, dDTF) in extended precision up to 132 signals and in
float64 NumPy beyond.  The chain of kernels changes with the signal count, and every size at which it does is here:

  1, 2, 3, 8 | 9, 11 | 12 ... (block size of the LDS kernels: mv_threads), 16 | 17, 32 | 33, 47, 48 (m_inverse_gj<1..4>, LU in LDS)
  49, 63, 64 (m_inverse_mfma<4>, m_gemm_mfma<6>), 65, 80, 96 (<6>), 97, 127, 128 (<8>)
  129, 130, 200, 256 (m_inverse_global<16, 256>, blocked products, m_measure without its LDS cache), 257, 300, 512 (<8, 512>)

(a) every quantity against the reference: max |got - ref| <= K_q 2^-52 max |ref|, both maxima per window.  K_q = 4 x the largest
    ratio measured on an MI355X over the cases of (a), rounded up to a power of two (profiles/mvar_measure_accuracy.txt, written
    by tools/mvar_measure_accuracy.py, with the ratio of the float64 NumPy evaluation of the same cases beside it).
(b) identities: DTF rows and PDC / gPDC columns sum to 1, Sigma exactly symmetric, two runs the same bits, and the H, A, Sigma
    outputs are what the measures were computed from.
(c) three windows of different scale: each to the bar of (a), permuted windows give permuted outputs, Sigma_p = L_p D_p^2 L_p^T.
(d) SC_MVAR_INVERSE: small16 / small32 / small64 move the first boundary, registers takes m_inverse_inplace<6 / 8>.
(e) ill-conditioned H0 / H (cond 1e6): the Tikhonov terms decide the answer, and the reference without them is rejected.
(f) N = 2 (H0 and its inverse fill the A buffer exactly), N = 32 (the partial sums follow the bins), one window, one signal.
(g) nothing is written outside the workspace or the output; a workspace one byte short is refused before anything runs.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvar_measures_ref as mref                                              # noqa: E402
from guarded_buffers import BAND, guarded, intact                             # noqa: E402
from spectral_connectivity_amd import _lib                                    # noqa: E402

gpu = pytest.mark.gpu

SIZES = [1, 2, 3, 8, 9, 11, 12, 16, 17, 32, 33, 47, 48, 49, 63, 64, 65, 80, 96, 97, 127, 128, 129, 130, 200, 256, 257, 300, 512]
KINDS = {"structured": mref.structured, "free": mref.free}
WHICH = dict(zip(mref.QUANTITIES, (_lib.MVAR_DTF, _lib.MVAR_DC, _lib.MVAR_PDC, _lib.MVAR_GPDC, _lib.MVAR_DDTF, _lib.MVAR_TRANSFER,
                                   _lib.MVAR_COEFFICIENTS, _lib.MVAR_NOISE_COVARIANCE)))
# profiles/mvar_measure_accuracy.txt: 4 x the largest device ratio of the quantity over the cases of (a), next power of two.  The maxima:
# DTF 6.43, DC 25.38, PDC 19.86, gPDC 15.00, dDTF 19.09, H 24.04, A 31.32 (all at 256 ... 512 signals, where the reference is float64
# NumPy with errors of its own: against the extended reference, up to 130 signals, the device stays below 4 / 13 / 4 / 11 / 10 / 13 / 19),
# Sigma 10.81.  The float64 NumPy evaluation of the same cases reaches 5 ... 12 up to 130 signals.
K = {"directed_transfer_function": 32.0, "directed_coherence": 128.0, "partial_directed_coherence": 128.0,
     "generalized_partial_directed_coherence": 64.0, "direct_directed_transfer_function": 128.0, "transfer_function": 128.0,
     "mvar_coefficients": 128.0, "noise_covariance": 64.0}


def shape_of(kind, C):
    """(N, P) of the cases of (a): 8 bins and 2 windows (3 for the small ``free`` cases), 4 bins from 257 signals on"""
    return (4, 2) if C >= 257 else (8, 3 if kind == "free" and C <= 64 else 2)


def _freeze(*dicts):
    for d in dicts:
        for a in d.values():
            a.setflags(write=False)


@functools.lru_cache(maxsize=6)
def case(kind, C, N, P):
    """(G, reference) of a case: computed once, shared, never written to."""
    G = KINDS[kind](C, N, P, 1000 + C)
    ref = mref.reference(G)
    G.setflags(write=False)
    _freeze(ref)
    return G, ref


def run_all(G, names=mref.QUANTITIES):
    """{quantity: array} from the device, every quantity its own call on one uploaded G"""
    import torch
    from spectral_connectivity_amd import engine
    _lib.require_gpu()
    d = torch.from_numpy(np.array(G, order="C")).to("cuda:0")
    out = {}
    for name in names:
        t = engine.mvar_measure(d, WHICH[name])
        P, N, C, _ = G.shape
        want = (P, C, C) if name == "noise_covariance" else (P, N // 2 + 1, C, C)
        assert tuple(t.shape) == want and t.dtype == (torch.complex128 if name in ("transfer_function", "mvar_coefficients") else torch.float64)
        out[name] = t.cpu().numpy()
    return out


@functools.lru_cache(maxsize=4)
def device_case(kind, C, N, P):
    got = run_all(case(kind, C, N, P)[0])
    _freeze(got)
    return got


def ratios(got, ref, scale=None):
    return {name: mref.ratio(got[name], ref[name], scale) for name in got}


def assert_within(got, ref, what, scale=None):
    r = ratios(got, ref, scale)
    print(f"\n  {what}: |got - ref| / (2^-52 max |ref|): " + ", ".join(f"{n} {v:.2f}" for n, v in r.items()))
    bad = {n: v for n, v in r.items() if not v <= K[n]}
    assert not bad, (what, bad)


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------------
def accuracy_row(kind, C):
    """(device ratios, float64 NumPy ratios or None where NumPy is the reference) of one case of (a), per quantity"""
    N, P = shape_of(kind, C)
    G, ref = case(kind, C, N, P)
    numpy_r = ratios(mref.evaluate(G, "float64"), ref) if C <= mref.EXTENDED_MAX else None
    return ratios(device_case(kind, C, N, P), ref), numpy_r


@gpu
@pytest.mark.parametrize("C", SIZES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_quantity_against_the_reference(kind, C):
    N, P = shape_of(kind, C)
    assert_within(device_case(kind, C, N, P), case(kind, C, N, P)[1], f"{kind} C = {C}")


# ---- (b) identities ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [5, 48, 64, 100, 130, 260])
def test_identities_of_the_outputs(C):
    """Sums to one: an entry of DTF / PDC / gPDC is a squared modulus over a sum of C of them, each entry within 4 roundings
    (square root, two divisions, the squares) and the sum, accumulated in order, within C roundings of the exact one -- so a row
    (column) adds up to 1 within (C + 4) 2^-52 (summed here in extended precision).  The measures recomputed on the host in
    extended precision from the downloaded H, A, Sigma agree to 8 x 2^-52 of the maximum: the three outputs are the values the
    measures were computed from."""
    G = case("structured", C, 8, 2)[0]
    got = device_case("structured", C, 8, 2)
    again = run_all(G)
    for name in mref.QUANTITIES:
        assert got[name].dtype == again[name].dtype and np.array_equal(got[name], again[name]), f"{name}: two runs differ"
    s = got["noise_covariance"]
    assert np.array_equal(s, s.swapaxes(-1, -2)), "Sigma is not exactly symmetric"
    tol = (C + 4) * mref.EPS
    for name, axis in (("directed_transfer_function", -1), ("partial_directed_coherence", -2), ("generalized_partial_directed_coherence", -2)):
        total = got[name].astype(mref.LD).sum(axis=axis)
        assert float(np.abs(total - 1).max()) <= tol, (name, float(np.abs(total - 1).max()) / mref.EPS)
    host = mref.measures_from(got["transfer_function"].astype(mref.CLD), got["mvar_coefficients"].astype(mref.CLD), s.astype(mref.LD))
    for name in ("directed_transfer_function", "generalized_partial_directed_coherence"):
        r = mref.ratio(got[name], host[name])
        print(f"\n  C = {C} {name} against the host's from the downloaded H, A, Sigma: {r:.2f} x 2^-52")
        assert r <= 8.0, (name, r)


# ---- (c) windows ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [5, 48, 64, 100, 130])
def test_three_windows_of_different_scale(C):
    """D_p scaled by 1, 4 and 7.  Every window on its own scale (mref.ratio), the windows in another order, and Sigma against
    the closed form L D^2 L^T: the device is within K of the extended evaluation, and that within 64 of the closed form
    (tests/test_mvar_measures_ref.py at these sizes), both in units of 2^-52 max |Sigma_p|."""
    G, ref = case("structured", C, 8, 3)
    got = device_case("structured", C, 8, 3)
    assert_within(got, ref, f"three windows, C = {C}")
    d = np.einsum("pii->p", ref["noise_covariance"]).astype(np.float64)
    assert d[1] > 4 * d[0] and d[2] > 1.5 * d[1], "the windows were to differ in scale"
    order = [2, 0, 1]
    assert_within(run_all(G[order]), {n: a[order] for n, a in ref.items()}, f"windows permuted, C = {C}")
    closed = mref.structured(C, 8, 3, 1000 + C, closed=True)[1]["noise_covariance"]
    r = mref.ratio(got["noise_covariance"], closed)
    print(f"  Sigma against L D^2 L^T: {r:.2f}")
    assert r <= K["noise_covariance"] + 64.0


# ---- (d) the switch ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("value,C", [("small16", 17), ("small32", 33), ("small32", 48), ("small64", 49), ("small64", 63), ("small64", 64),
                                     ("registers", 70), ("registers", 96), ("registers", 100), ("registers", 128)])
def test_inverse_variants(debug_env, value, C):
    """SC_MVAR_INVERSE selects another kernel chain for the same algebra: the bar of (a) against the reference, and against
    what the default chain gives (two results within K / 4 of the reference each, by the rule K was set with)."""
    G, ref = case("structured", C, 8, 2)
    default = run_all(G)
    debug_env("SC_MVAR_INVERSE", value)
    got = run_all(G)
    debug_env("SC_MVAR_INVERSE", None)
    assert_within(got, ref, f"SC_MVAR_INVERSE={value}, C = {C}")
    assert_within(got, {n: a.astype(mref.CLD if np.iscomplexobj(a) else mref.LD) for n, a in default.items()}, f"{value} against the default, C = {C}")
    assert any(not np.array_equal(got[n], default[n]) for n in ("transfer_function", "mvar_coefficients")), "the switch selected nothing"


# ---- (e) Tikhonov --------------------------------------------------------------------------------------------------------------------
# Sizes: 6, 20 and the largest of 49 ... 64 and 65 ... 128 at which the case meets the factor 8 of
# test_mvar_measures_ref.py::test_tikhonov_cases_are_sensitive.  where = "h0": lam = 1e-12 mean(H0^2) is set by the large windows
# beside the modified one and stays worth hundreds of tolerances up to 128 signals.  where = "h": lam' = 1e-12 mean(|H|^2) with
# |H| ~ 1 moves A by lam' cond |v^H u| (u, v: the singular vectors of the small singular value), which falls like C^-3/2 against a
# tolerance of K_A 2^-52 cond: 8.0 tolerances at 6 signals, 1.2 at 20, 0.14 at 64, 0.05 at 128 -- the sizes that do not reach the
# factor 8 are left out (TIKHONOV_DROPPED), the factor stays.
TIKHONOV_OUTPUTS = ("transfer_function", "mvar_coefficients", "directed_transfer_function")
TIKHONOV_CASES = [("h0", 6), ("h0", 20), ("h0", 64), ("h0", 128), ("h", 6)]
TIKHONOV_DROPPED = [("h", 20), ("h", 64), ("h", 128)]


@functools.lru_cache(maxsize=2)
def tikhonov_case(where, C):
    """(G, extended reference with the lam terms, without them)"""
    G = mref.tikhonov(C, 8, 2, 500 + C, where)
    with_lam, without = mref.evaluate(G, "extended"), mref.evaluate(G, "extended", tikhonov=False)
    G.setflags(write=False)
    _freeze(with_lam, without)
    return G, with_lam, without


def tikhonov_scale(ref):
    """per-window multipliers of the bar: the condition number for the modified window, 1 for the others"""
    s = np.ones(ref.shape[0])
    s[mref.TIKHONOV_WINDOW] = mref.TIKHONOV_COND
    return s


def tikhonov_miss(got, ref):
    """{output: |got - ref| of the MODIFIED window alone in units of that window's tolerance} (the other windows are plain
    ``structured`` ones, whose H0 -- noise variances over five decades -- feels lam too: they must not carry the case)"""
    w = slice(mref.TIKHONOV_WINDOW, mref.TIKHONOV_WINDOW + 1)
    return {n: mref.ratio(got[n][w], ref[n][w], [mref.TIKHONOV_COND]) / K[n] for n in TIKHONOV_OUTPUTS}


@gpu
@pytest.mark.parametrize("where,C", TIKHONOV_CASES)
def test_tikhonov_terms_decide(where, C):
    G, with_lam, without = tikhonov_case(where, C)
    got = run_all(G, TIKHONOV_OUTPUTS)
    scale = tikhonov_scale(with_lam["transfer_function"])
    assert_within(got, {n: with_lam[n] for n in got}, f"Tikhonov {where}, C = {C}", scale)
    miss = tikhonov_miss(got, without)
    print("  modified window against the reference without the lam terms, in tolerances: " + ", ".join(f"{n} {v:.1f}" for n, v in miss.items()))
    assert max(miss.values()) > 1.0, "the reference without the Tikhonov terms passes too: the case has lost its meaning"


# ---- (f) edges -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,C,N,P", [("structured", 70, 2, 2), ("free", 70, 2, 3), ("structured", 12, 32, 2), ("free", 12, 32, 2),
                                        ("structured", 20, 8, 1), ("structured", 70, 8, 1), ("free", 130, 4, 1),
                                        ("structured", 1, 2, 1), ("free", 1, 8, 3)])
def test_edges(kind, C, N, P):
    """N = 2 beyond 48 signals: H0 and its inverse, parked in the A buffer (2 P C^2 elements), fill its P (N / 2 + 1) C^2 exactly.
    N = 32 at 12 signals: 17 partial sums per window where 16 are reserved at least.  One window; one signal."""
    G, ref = case(kind, C, N, P)
    assert_within(run_all(G), ref, f"{kind} C = {C}, N = {N}, P = {P}")


# ---- (g) stores ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [5, 64, 100, 130, 260])
def test_nothing_is_stored_outside_the_buffers(C):
    """The workspace of exactly sc_mvar_workspace_bytes bytes and the output, each between two 4 KB bands of a pattern: the bands
    survive each of the eight calls and the outputs are those of engine.mvar_measure.  With one byte less the call is refused,
    and neither the workspace nor the output is touched."""
    import torch
    from spectral_connectivity_amd import engine
    lib = _lib._handle()
    N, P = (4, 2) if C > 128 else (8, 2)
    G = case("structured", C, N, P)[0]
    F = N // 2 + 1
    d_G = torch.from_numpy(np.array(G, order="C")).to("cuda:0")
    nbytes = ctypes.c_size_t()
    _lib.check(lib.sc_mvar_workspace_bytes(P, C, N, ctypes.byref(nbytes)), "sc_mvar_workspace_bytes")
    nbytes = nbytes.value
    stream = engine.TorchMemory(d_G.device).stream()

    for name in mref.QUANTITIES:
        itemsize = 16 if name in ("transfer_function", "mvar_coefficients") else 8
        count = P * C * C if name == "noise_covariance" else P * F * C * C
        out, work = guarded(count * itemsize), guarded(nbytes)
        args = (ctypes.c_void_p(d_G.data_ptr()), P, N, C, WHICH[name], ctypes.c_void_p(out.data_ptr() + BAND),
                ctypes.c_void_p(work.data_ptr() + BAND))
        rc = lib.sc_mvar_measure_f64(*args, nbytes - 1, stream)
        torch.cuda.synchronize()
        assert rc != 0, "a workspace one byte short was accepted"
        assert bool((out[BAND:BAND + count * itemsize] == 0x5A).all()) and bool((work[BAND:BAND + nbytes] == 0x5A).all()), "a refused call wrote"
        _lib.check(lib.sc_mvar_measure_f64(*args, nbytes, stream), "sc_mvar_measure_f64")
        torch.cuda.synchronize()
        assert intact(out, count * itemsize), f"{name}: stored outside the output"
        assert intact(work, nbytes), f"{name}: stored outside the workspace"
        want = engine.mvar_measure(d_G, WHICH[name])
        mine = out[BAND:BAND + count * itemsize].view(want.dtype).view(want.shape)
        assert torch.equal(mine, want), name
