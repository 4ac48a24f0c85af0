"""Conditional spectral Granger prediction: time of the call on top of the cached full factor, 7 windows x 256 bins.
Usage: python tools/conditional_granger_time.py [C ...] [--ref].  --ref also times the NumPy float64 reference
(tests/conditional_granger_ref.py, closed form on the oracle's Wilson iteration) on the same spectra and compares.
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split (cg_gather / cg_epilogue against the Wilson kernels)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spectral_connectivity_amd as sc      # noqa: E402
from spectral_connectivity_amd import _lib   # noqa: E402

sizes = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [8, 32, 64, 128]
W, L, R = 7, 256, 40      # 200 observations a window: more than the signals, or the spectra are singular
for C in sizes:
    rng = np.random.default_rng(9)
    T = W * L
    e = rng.standard_normal((T + 100, R, C))
    x = np.zeros_like(e)
    for t in range(2, T + 100):
        x[t] = 0.45 * x[t - 1] - 0.25 * x[t - 2] + e[t]
        x[t, :, 1:] += 0.3 * x[t - 1, :, :-1]
    x = x[100:]
    m = sc.Multitaper(x, sampling_frequency=500.0, time_halfbandwidth_product=3, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    for rep in range(2):
        c = sc.Connectivity.from_multitaper(m)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c._mvar_factor_device()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _lib.timing_enable(True)
        _lib.last_timing()
        out = c.conditional_spectral_granger_prediction()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        timers = _lib.last_timing()
        _lib.timing_enable(False)
    lw = c._last_wilson
    factor_ms = sum(v for k, v in timers if k == "mvar_factor")
    total_ms = sum(v for k, v in timers if k == "conditional_granger")
    print(f"C={C} {W} windows x {L} bins: full factor {1e3 * (t1 - t0):.1f} ms; conditional call {1e3 * (t2 - t1):.1f} ms "
          f"(library: {total_ms:.1f} ms, of which reduced Wilson {factor_ms:.1f} ms in {sum(k == 'mvar_factor' for k, _ in timers)} "
          f"chunk(s)); reduced iterations {lw['iterations']}, not converged {lw['not_converged']}; finite {np.isfinite(out).mean():.2f}",
          flush=True)
    if "--ref" in sys.argv and C == sizes[0]:      # (the reference's Wilson iteration is slow beyond a few signals)
        import conditional_granger_ref as cref
        from oracle import spectral_oracle as so
        coef, _ = so.multitaper_fft(x, fs=500.0, NW=3, n_time_samples_per_window=L, n_time_samples_per_step=L)
        S = so.expectation_csm_gemm(coef, "trials_tapers")
        t0 = time.perf_counter()
        ref = cref.conditional_granger_closed(S)
        t1 = time.perf_counter()
        both = np.isfinite(ref) & np.isfinite(out)
        print(f"  NumPy reference {1e3 * (t1 - t0):.0f} ms; max |device - reference| {np.abs(out - ref)[both].max():.2e}", flush=True)
