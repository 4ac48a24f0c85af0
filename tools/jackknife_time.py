"""Device time of the delete-one jackknife (sc_jackknife.hip) beside coherence_magnitude() on the same complex spectra, both
engines, and beside the alternative without it: n_trials Connectivity passes over the n_trials - 1 other trials each.

    python tools/jackknife_time.py                  # headline shape: 128 channels, 1000 trials, 7 tapers, 7 windows, 129 bins
    python tools/jackknife_time.py --loop           # 128 channels x 32 trials: the kernel against the leave-one-out loop
    python tools/jackknife_time.py --one            # one call at the headline shape (for rocprofv3 --kernel-trace --stats)
Optional: --channels C --trials R.  Times are hipEvent intervals around the engine calls (spectra resident, best of 3)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc                  # noqa: E402
from spectral_connectivity_amd import _lib, engine      # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, reps=3):
    best, out = 1e30, None
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


def spectra(C, R, dtype, W=7, L=256):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((W * L, R, C), generator=g, device="cuda", dtype=torch.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    m = sc.Multitaper(x.cpu().numpy(), sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    del x
    c = sc.Connectivity.from_multitaper(m, expectation_type="trials_tapers", dtype=dtype)
    return c, c._device()             # (no planes hint: complex64 / complex128 spectra)


def coherence(sp, n_freq):
    accum, n_obs = engine.accumulate(sp, "trials_tapers", _lib.PLANE_CSM, n_freq=n_freq)
    return engine.measure(accum, sp.C, _lib.PLANE_CSM, n_obs, _lib.M_COHERENCE_MAGNITUDE)


def jackknife(sp, n_freq, mask, over):
    total, n_obs = engine.accumulate(sp, "trials_tapers", _lib.PLANE_CSM, n_freq=n_freq)
    n_units = sp.R if over == 0 else n_obs
    return engine.jackknife(sp, "trials_tapers", total, _lib.PLANE_CSM, mask, over, n_units, n_freq=n_freq)[0]


def headline(C, R):
    for dtype, name in ((np.complex64, "float32 engine"), (np.complex128, "float64 engine")):
        c, sp = spectra(C, R, dtype)
        F = c._n_freq
        t_coh, _ = timed(lambda: coherence(sp, F))
        print(f"{name}: {C} channels, {R} trials, {sp.K} tapers, {sp.W} windows, {F} bins: coherence_magnitude {t_coh:.2f} ms", flush=True)
        for what, mask, over in (("jackknife coherence_magnitude", 0x2, 0), ("jackknife all three measures", 0x7, 0),
                                 ("jackknife coherence_magnitude over observations", 0x2, 1)):
            t, _ = timed(lambda: jackknife(sp, F, mask, over))
            print(f"    {what}: {t:.2f} ms (total record included), {t / t_coh:.2f} x coherence_magnitude", flush=True)
        del c, sp
        torch.cuda.empty_cache()


def loop(C, R):
    for dtype, name in ((np.complex64, "float32 engine"), (np.complex128, "float64 engine")):
        c, sp = spectra(C, R, dtype)
        F = c._n_freq
        X = sp.X.view(sp.F, sp.W, sp.R, sp.K, sp.C_alloc)

        def leave_one_out_passes():
            outs = []
            for r in range(R):
                keep = torch.cat([torch.arange(0, r, device=X.device), torch.arange(r + 1, R, device=X.device)])
                sub = X.index_select(2, keep)                           # gather on the device
                st = (sp.W * (R - 1) * sp.K * sp.C_alloc, (R - 1) * sp.K * sp.C_alloc, sp.K * sp.C_alloc, sp.C_alloc)
                one = engine.DeviceSpectra(sub, (sp.F, sp.W, R - 1, sp.K, sp.C), st, sp.n_fft, True, C_alloc=sp.C_alloc)
                outs.append(coherence(one, F))
            return outs

        t_loop, _ = timed(leave_one_out_passes)
        t_jk, _ = timed(lambda: jackknife(sp, F, 0x2, 0))
        print(f"{name}: {C} channels x {R} trials: {R} leave-one-out Connectivity passes {t_loop:.2f} ms, device jackknife "
              f"{t_jk:.2f} ms, ratio {t_loop / t_jk:.1f}", flush=True)
        del c, sp, X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--loop" in sys.argv:
        loop(arg("--channels", 128), arg("--trials", 32))
    elif "--one" in sys.argv:
        c, sp = spectra(arg("--channels", 128), arg("--trials", 1000), np.complex64)
        jackknife(sp, c._n_freq, 0x7, 0)
        torch.cuda.synchronize()
    else:
        headline(arg("--channels", 128), arg("--trials", 1000))
