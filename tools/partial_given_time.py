"""Device time of partial and multiple coherence given a chosen set of signals (sc_partial_coherence_given_f64, all three outputs)
for 7 windows x 129 bins = 903 problems of a kept signals given m, on float32 and float64 records of a + m signals from 224
observations, beside what a user has without it: torch.linalg.solve on the same 903 complex128 given blocks plus the elementwise
epilogue, on the same GPU.  The solve is against the identity (m right-hand sides) and S_ZA is multiplied in afterwards: handed
S_ZA itself at 6 given and 300 kept signals -- 903 systems of 6 x 6 with 300 right-hand sides -- the batched solve of the PyTorch
build this was measured with ended in a HIP launch failure.

    python tools/partial_given_time.py                  # the table of profiles/partial_given_time.txt
    python tools/partial_given_time.py --only 300 6     # that row alone
    python tools/partial_given_time.py --one            # one call at 300 kept given 6 (for rocprofv3 --kernel-trace --stats)
    SC_HIP_LIB=<variant> python tools/partial_given_time.py --steps n
                                                        # the kernel alone, from a library built with -DPC_STEPS=n
                                                        # (_build.build(extra_flags=["-DPC_STEPS=n"], out=<variant>)): the
                                                        # problem ends after step n, differences of the rows = time per step
Times are hipEvent intervals around the calls (records and matrices resident, best of 5).  The store rate of a row is the bytes of
the three outputs over the whole time of the call."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc                  # noqa: E402
from spectral_connectivity_amd import _lib, engine      # noqa: E402

WANT = ("coherency", "magnitude", "multiple")
SIZES = ((62, 2), (126, 2), (64, 64), (14, 128), (300, 6), (512, 16))
HBM_TB_S = 6.3                  # achievable HBM3E rate of an MI355X (8 TB/s peak)


def timed(fn, reps=5):
    best, out = 1e30, None
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


def records(C, dtype, W=7, L=256, R=32):
    """(CSM records [W * 129, ...] of C signals over R trials x 7 tapers = 224 observations, n_obs)."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((W * L, R, C), generator=g, device="cuda", dtype=torch.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    m = sc.Multitaper(x.cpu().numpy(), sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    c = sc.Connectivity.from_multitaper(m, expectation_type="trials_tapers", dtype=dtype)
    accum, n_obs = engine.accumulate(c._device(), "trials_tapers", _lib.PLANE_CSM, n_freq=c._n_freq)
    return accum, n_obs


def matrices(accum, C, n_obs):
    """The cross-spectral matrices [n_bins, C, C] complex128 the records hold (include/sc_hip.h: planes Re, Im of upper-triangular
    16 x 16 channel tiles, tile (bi, bj) at bi NB - bi (bi - 1) / 2 + (bj - bi))."""
    NB = (C + 15) // 16
    n_tiles = NB * (NB + 1) // 2
    rec = accum.reshape(accum.shape[0], 2, n_tiles, 16, 16).to(torch.float64)
    S = torch.zeros((accum.shape[0], NB * 16, NB * 16), dtype=torch.complex128, device=accum.device)
    for bi in range(NB):
        for bj in range(bi, NB):
            t = bi * NB - bi * (bi - 1) // 2 + (bj - bi)
            S[:, bi * 16:(bi + 1) * 16, bj * 16:(bj + 1) * 16] = torch.complex(rec[:, 0, t], rec[:, 1, t])
    S = torch.triu(S)
    d = torch.diagonal(S, dim1=-2, dim2=-1).real
    S = S + torch.triu(S, 1).conj().transpose(-1, -2)
    S[:, torch.arange(NB * 16), torch.arange(NB * 16)] = torch.complex(d, torch.zeros_like(d))
    return (S[:, :C, :C] / n_obs).contiguous()


def lists(a, m):
    """Kept: a sorted random subset; given: a random subset in random order (the layout of the GPU tests)."""
    perm = np.random.default_rng(a + m).permutation(a + m)
    return np.sort(perm[m:]).astype(np.int32), perm[:m].astype(np.int32)


def solve_and_epilogue(S, kept, given):
    k, z = torch.as_tensor(kept.astype(np.int64), device=S.device), torch.as_tensor(given.astype(np.int64), device=S.device)
    Szz, Sza, Saa = S[:, z][:, :, z], S[:, z][:, :, k], S[:, k][:, :, k]
    eye = torch.eye(len(given), dtype=S.dtype, device=S.device).expand(S.shape[0], -1, -1)
    E = Saa - Sza.conj().transpose(-1, -2) @ (torch.linalg.solve(Szz, eye) @ Sza)
    e = torch.diagonal(E, dim1=-2, dim2=-1).real
    s = torch.diagonal(Saa, dim1=-2, dim2=-1).real
    coherency = E / torch.sqrt(e[:, :, None] * e[:, None, :])
    return coherency, coherency.abs(), torch.sqrt(torch.clamp(1.0 - e / s, min=0.0))


def table(sizes=SIZES):
    print("903 problems (7 windows x 129 bins), all three outputs; ms, best of 5; output GB/s = bytes of the outputs / time")
    print(f"{'kept':>5} {'given':>5} {'records':>8} {'LDS bytes':>10} {'sc_partial_coherence_given_f64':>31} {'torch.linalg.solve + epilogue':>30} "
          f"{'worst |difference|':>19} {'output GB/s':>12} {'of HBM':>7}")
    lib = _lib.load()
    for a, m in sizes:
        C = a + m
        kept, given = lists(a, m)
        for dtype, name in ((np.complex64, "float32"), (np.complex128, "float64")):
            accum, n_obs = records(C, dtype)
            t_dev, (res, counts) = timed(lambda: engine.partial_coherence_given(accum, C, _lib.PLANE_CSM, n_obs, kept, given, WANT))
            S = matrices(accum, C, n_obs)
            t_ref, ref = timed(lambda: solve_and_epilogue(S, kept, given))
            off = ~torch.eye(a, dtype=torch.bool, device=S.device)
            diff = max((res["coherency"] - ref[0])[:, off].abs().max().item(), (res["multiple"] - ref[2]).abs().max().item())
            out_bytes = accum.shape[0] * (24 * a * a + 8 * a)
            rate = out_bytes / (t_dev * 1e-3) / 1e9
            print(f"{a:>5} {m:>5} {name:>8} {lib.sc_partial_given_lds_bytes(a, m):>10} {t_dev:>31.3f} {t_ref:>30.3f} {diff:>19.2e} "
                  f"{rate:>12.0f} {rate / (HBM_TB_S * 1e3):>7.1%}   (fail counters {counts})", flush=True)
            del accum, S, res, ref
            torch.cuda.empty_cache()
    print(f"192 kept given 128: {lib.sc_partial_given_lds_bytes(192, 128)} bytes of LDS, beyond the {lib.sc_partial_given_lds_limit()} "
          "of a compute unit -- not served (ValueError)")


def steps(n):
    for a, m in ((64, 64), (14, 128), (300, 6)):
        kept, given = lists(a, m)
        accum, n_obs = records(a + m, np.complex128)
        t, _ = timed(lambda: engine.partial_coherence_given(accum, a + m, _lib.PLANE_CSM, n_obs, kept, given, WANT))
        print(f"steps 1..{n}: {a:>4} kept given {m:>3}, float64 records: {t:.3f} ms", flush=True)


if __name__ == "__main__":
    if "--one" in sys.argv:
        kept, given = lists(300, 6)
        accum, n_obs = records(306, np.complex128)
        engine.partial_coherence_given(accum, 306, _lib.PLANE_CSM, n_obs, kept, given, WANT)
        torch.cuda.synchronize()
    elif "--steps" in sys.argv:
        steps(int(sys.argv[sys.argv.index("--steps") + 1]))
    elif "--only" in sys.argv:
        at = sys.argv.index("--only")
        table(((int(sys.argv[at + 1]), int(sys.argv[at + 2])),))
    else:
        table()
