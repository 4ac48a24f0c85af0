"""Blockwise spectral Granger prediction: time of the call, 7 windows x 256 bins, float64 engine.
Usage: python tools/blockwise_granger_time.py [n_blocks:block_size ...] [--ref].  Default 8:16 (128 signals, 28 block pairs of 32);
2:128 times the epilogue's in-place path (blocks of more than 64 signals).
--ref also times the NumPy float64 reference (tests/blockwise_granger_ref.py, null-space form on the oracle's Wilson iteration)
on the same spectra and compares.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel split (bw_gather /
bw_nullspace / bw_epilogue and the product against the Wilson kernels)."""
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

cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:] if not a.startswith("--")] or [(8, 16)]
W, L = 7, 256
for n_blocks, size in cases:
    C = n_blocks * size
    R = max(40, -(-(2 * size + 8) // 5))     # trials x 5 tapers: more observations than the signals of a pair, or its spectra are singular
    rng = np.random.default_rng(9)
    T = W * L
    e = rng.standard_normal((T + 100, R, C))
    x = np.zeros_like(e)
    for t in range(2, T + 100):
        x[t] = 0.45 * x[t - 1] - 0.25 * x[t - 2] + e[t]
        x[t, :, 1:] += 0.3 * x[t - 1, :, :-1]
    x = x[100:]
    labels = np.arange(C) // size
    m = sc.Multitaper(x, sampling_frequency=500.0, time_halfbandwidth_product=3, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    for rep in range(2):
        c = sc.Connectivity.from_multitaper(m)
        c._csm_records("granger")
        torch.cuda.synchronize()
        _lib.timing_enable(True)
        _lib.last_timing()
        t0 = time.perf_counter()
        out, _ = c.blockwise_spectral_granger_prediction(labels)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        timers = _lib.last_timing()
        _lib.timing_enable(False)
    lw = c._last_wilson
    factor_ms = sum(v for k, v in timers if k == "mvar_factor")
    total_ms = sum(v for k, v in timers if k == "blockwise_granger")
    print(f"{n_blocks} blocks x {size} signals, {W} windows x {L} bins, {R} trials: call {1e3 * (t1 - t0):.1f} ms (library: {total_ms:.1f} ms, "
          f"of which Wilson {factor_ms:.1f} ms in {sum(k == 'mvar_factor' for k, _ in timers)} batch(es); ratio "
          f"{total_ms / max(factor_ms, 1e-9):.3f}); iterations {lw['iterations']}, not converged {lw['not_converged']}; "
          f"finite {np.isfinite(out).mean():.2f}", flush=True)
    if "--ref" in sys.argv and (n_blocks, size) == cases[0]:
        import blockwise_granger_ref as bref
        from oracle import spectral_oracle as so
        coef, _ = so.multitaper_fft(x, fs=500.0, NW=3, n_time_samples_per_window=L, n_time_samples_per_step=L)
        S = so.expectation_csm_gemm(coef, "trials_tapers")
        t0 = time.perf_counter()
        ref, _ = bref.blockwise_granger(S, labels)
        t1 = time.perf_counter()
        both = np.isfinite(ref) & np.isfinite(out)
        print(f"  NumPy reference {1e3 * (t1 - t0):.0f} ms; max |device - reference| {np.abs(out - ref)[both].max():.2e}", flush=True)
