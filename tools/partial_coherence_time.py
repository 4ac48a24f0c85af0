"""Device time of partial and multiple coherence (sc_partial_coherence_f64, all three outputs) for 7 windows x 129 bins = 903
cross-spectral matrices of 16, 64 and 128 signals, on float32 and float64 records, beside what a user has without it:
torch.linalg.inv of the same 903 complex128 matrices plus the elementwise epilogue, on the same GPU.

    python tools/partial_coherence_time.py                  # the table of profiles/partial_coherence_time.txt
    python tools/partial_coherence_time.py --one            # one call at 128 signals (for rocprofv3 --kernel-trace --stats)
    SC_HIP_LIB=<variant> python tools/partial_coherence_time.py --steps n
                                                            # the kernel alone, from a library built with -DPC_STEPS=n
                                                            # (_build.build(extra_flags=["-DPC_STEPS=n"], out=<variant>)): the
                                                            # problem ends after step n, differences of the rows = time per step
Times are hipEvent intervals around the calls (records and matrices resident, best of 5)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc                  # noqa: E402
from spectral_connectivity_amd import _lib, engine      # noqa: E402

WANT = ("coherency", "magnitude", "multiple")


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
    """(CSM records [W * 129, ...] over R trials x 7 tapers = 224 observations, n_obs, the same matrices [903, C, C] complex128)."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((W * L, R, C), generator=g, device="cuda", dtype=torch.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    m = sc.Multitaper(x.cpu().numpy(), sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    c = sc.Connectivity.from_multitaper(m, expectation_type="trials_tapers", dtype=dtype)
    sp = c._device()
    accum, n_obs = engine.accumulate(sp, "trials_tapers", _lib.PLANE_CSM, n_freq=c._n_freq)
    X = sp.coefficients().to(torch.complex128)[:c._n_freq]                          # (F, W, R, K, C)
    S = torch.einsum("fwrki,fwrkj->wfij", X, X.conj()).reshape(-1, C, C) / n_obs
    return accum, n_obs, S.contiguous()


def inverse_and_epilogue(S):
    G = torch.linalg.inv(S)
    g = torch.diagonal(G, dim1=-2, dim2=-1).real
    s = torch.diagonal(S, dim1=-2, dim2=-1).real
    coherency = -G / torch.sqrt(g[:, :, None] * g[:, None, :])
    return coherency, coherency.abs(), torch.sqrt(torch.clamp(1.0 - 1.0 / (s * g), min=0.0))


def table():
    print("903 matrices (7 windows x 129 bins), all three outputs; ms, best of 5")
    print(f"{'signals':>8} {'records':>8} {'sc_partial_coherence_f64':>25} {'torch.linalg.inv + epilogue':>28} {'worst |difference|':>19}")
    for C in (16, 64, 128):
        for dtype, name in ((np.complex64, "float32"), (np.complex128, "float64")):
            accum, n_obs, S = records(C, dtype)
            t_dev, (res, n_fail) = timed(lambda: engine.partial_coherence(accum, C, _lib.PLANE_CSM, n_obs, WANT))
            t_inv, ref = timed(lambda: inverse_and_epilogue(S))
            off = ~torch.eye(C, dtype=torch.bool, device=S.device)
            diff = max((res["coherency"] - ref[0])[:, off].abs().max().item(), (res["multiple"] - ref[2]).abs().max().item())
            print(f"{C:>8} {name:>8} {t_dev:>25.3f} {t_inv:>28.3f} {diff:>19.2e}   (n_fail {n_fail})", flush=True)
            del accum, S, res, ref
            torch.cuda.empty_cache()


def steps(n):
    for C in (16, 64, 128):
        accum, n_obs, _ = records(C, np.complex128)
        t, _ = timed(lambda: engine.partial_coherence(accum, C, _lib.PLANE_CSM, n_obs, WANT))
        print(f"steps 1..{n}: {C:>4} signals, float64 records: {t:.3f} ms", flush=True)


if __name__ == "__main__":
    if "--one" in sys.argv:
        accum, n_obs, _ = records(128, np.complex128)
        engine.partial_coherence(accum, 128, _lib.PLANE_CSM, n_obs, WANT)
        torch.cuda.synchronize()
    elif "--steps" in sys.argv:
        steps(int(sys.argv[sys.argv.index("--steps") + 1]))
    else:
        table()
