"""Device time of the delete-one jackknife of the phase-lag family (jk_phase_kernel and jk_phase_totals_kernel of sc_jackknife.hip)
beside the jackknife of the imaginary coherence on the same complex spectra, both engines, and beside the alternative without it:
n_trials Connectivity passes of weighted_phase_lag_index() over the n_trials - 1 other trials each.

    python tools/phase_lag_jackknife_time.py            # headline shape (128 channels, 1000 trials, 7 tapers, 7 windows, 129 bins),
                                                        # then 128 channels x 32 trials against the leave-one-out loop
    python tools/phase_lag_jackknife_time.py --one      # one call at the headline shape (for rocprofv3 --kernel-trace --stats)
Optional: --channels C --trials R --loop-trials R.  Times are hipEvent intervals around the engine calls (spectra resident, best of
5); the result goes to profiles/phase_lag_jackknife_time.txt as well (--out PATH for another file)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc                  # noqa: E402
from spectral_connectivity_amd import _lib, engine      # noqa: E402

WPLI = _lib.JACKKNIFE_PHASE_MEASURES["weighted_phase_lag_index"][0]
ALL_FOUR = 0xF
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


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


def spectra(C, R, dtype, W=7, L=256):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((W * L, R, C), generator=g, device="cuda", dtype=torch.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    m = sc.Multitaper(x.cpu().numpy(), sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    del x
    c = sc.Connectivity.from_multitaper(m, expectation_type="trials_tapers", dtype=dtype)
    return c, c._device()             # (no planes hint: complex64 / complex128 spectra)


def planes_of(mask):
    planes = 0
    for name, (bit, _, _) in _lib.JACKKNIFE_PHASE_MEASURES.items():
        if mask & bit:
            planes |= _lib.JACKKNIFE_PHASE_PLANES[name]
    return planes


def totals(sp, n_freq, mask):
    return engine.jackknife_phase_totals(sp, "trials_tapers", planes_of(mask), 0, n_freq=n_freq)[0]


def phase_jackknife(sp, n_freq, mask, total=None):
    """Totals pass (unless ``total`` is at hand) and jackknife pass."""
    total = totals(sp, n_freq, mask) if total is None else total
    return engine.jackknife_phase(sp, "trials_tapers", total, planes_of(mask), mask, 0, sp.R, n_freq=n_freq)[0]


def imaginary_coherence_jackknife(sp, n_freq):
    total, _ = engine.accumulate(sp, "trials_tapers", _lib.PLANE_CSM, n_freq=n_freq)
    return engine.jackknife(sp, "trials_tapers", total, _lib.PLANE_CSM, 0x4, 0, sp.R, n_freq=n_freq)[0]


def wpli(sp, n_freq):
    planes = _lib.PLANE_CSM | _lib.PLANE_ABS_IM
    accum, n_obs = engine.accumulate(sp, "trials_tapers", planes, n_freq=n_freq)
    return engine.measure(accum, sp.C, planes, n_obs, _lib.M_WPLI)


def headline(C, R):
    say(f"# headline shape, MI355X; hipEvent intervals around the engine calls, spectra resident, best of 5")
    for dtype, name in ((np.complex64, "float32 engine"), (np.complex128, "float64 engine")):
        c, sp = spectra(C, R, dtype)
        F = c._n_freq
        t_im, _ = timed(lambda: imaginary_coherence_jackknife(sp, F))
        say(f"{name}: {C} channels, {R} trials, {sp.K} tapers, {sp.W} windows, {F} bins: jackknife imaginary_coherence "
            f"{t_im:.2f} ms (total record included)")
        for what, mask in (("weighted_phase_lag_index", WPLI), ("all four phase-lag measures", ALL_FOUR)):
            t_tot, total = timed(lambda: totals(sp, F, mask))
            t_pass, _ = timed(lambda: phase_jackknife(sp, F, mask, total))
            t_both, _ = timed(lambda: phase_jackknife(sp, F, mask))
            say(f"    jackknife {what}: {t_both:.2f} ms (totals pass {t_tot:.2f} ms + jackknife pass {t_pass:.2f} ms), "
                f"{t_both / t_im:.2f} x the imaginary coherence's")
            del total
        del c, sp
        torch.cuda.empty_cache()


def loop(C, R):
    say(f"# the alternative without the kernel: n_trials Connectivity passes of weighted_phase_lag_index() over the other trials "
        f"(gather on the device)")
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
                outs.append(wpli(one, F))
            return outs

        t_loop, _ = timed(leave_one_out_passes)
        t_jk, _ = timed(lambda: phase_jackknife(sp, F, WPLI))
        say(f"{name}: {C} channels x {R} trials: {R} leave-one-out Connectivity passes {t_loop:.2f} ms, device jackknife "
            f"(totals pass included) {t_jk:.2f} ms, ratio {t_loop / t_jk:.1f}")
        del c, sp, X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--one" in sys.argv:
        c, sp = spectra(arg("--channels", 128), arg("--trials", 1000), np.complex64)
        phase_jackknife(sp, c._n_freq, ALL_FOUR)
        torch.cuda.synchronize()
    else:
        headline(arg("--channels", 128), arg("--trials", 1000))
        say("")
        loop(arg("--channels", 128), arg("--loop-trials", 32))
        out = arg("--out", os.path.join(ROOT, "profiles", "phase_lag_jackknife_time.txt"), str)
        with open(out, "w") as f:
            f.write("# tools/phase_lag_jackknife_time.py\n" + "\n".join(LINES) + "\n")
