"""What the amplitude guard of the float32 engine costs, and the float64 transform with its pair normalisation.

    python tools/amplitude_guard_time.py [--root TREE] [--f64-only]

Guard: for a fresh spectra object, a float32 request with s/|s| or (Im s)^2 pays one reduction over the complex64 spectra and one
small read-back before stage B.  Timed with device events around the scan and the host clock around scan + read-back, next to the
stage-B call it precedes (PLV's unit plane, the debiased wPLI's cross family), at 128 channels x 200 trials x 1024 samples.
Float64 transform: engine.multitaper_spectra_f64 at 64 channels x 200 trials, windows of 256 and 1024 samples (the radix-16
kernel; N = 1024 is the instantiation with the most registers).  ``--root``: time another checkout's package with this script."""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--f64-only", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

from spectral_connectivity_amd import Multitaper, _lib, engine  # noqa: E402


def device_ms(fn, repeats=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


rng = np.random.default_rng(0)
for L in (256, 1024):
    x = rng.standard_normal((4 * L, 200, 64))
    m = Multitaper(x, sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L, n_time_samples_per_step=L // 2)
    xd = torch.from_numpy(x).cuda()
    h = torch.from_numpy(np.ascontiguousarray(np.asarray(m.tapers).T / 1000.0)).cuda()
    ms = device_ms(lambda: engine.multitaper_spectra_f64(xd, h, L, L // 2, m.n_fft_samples, m.n_time_windows, "constant"))
    print(f"float64 transform  L={L:5d}  64 ch x 200 trials x {4 * L} samples  {ms:8.3f} ms")
    del xd, h
if args.f64_only:
    sys.exit(0)

x = rng.standard_normal((1024, 200, 128)).astype(np.float32)
m = Multitaper(x, sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=256, n_time_samples_per_step=128)
sp = m.device_spectra(precision="float32")
gb = sp.X.numel() * 8 / 1e9
for name, planes in (("s/|s| (PLV, PPC)", _lib.PLANE_UNIT), ("CSM + |Im s| + (Im s)^2 (debiased wPLI)", _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ)):
    def scan():
        sp._amplitude = None
        return engine.out_of_range(sp, planes)
    scan()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        scan()
    wall = (time.perf_counter() - t0) / 10 * 1e3
    stage_b = device_ms(lambda: engine.accumulate(sp, "trials_tapers", planes, guard=False))
    print(f"{name}: spectra {gb:.2f} GB  scan + read-back {wall:7.3f} ms (host clock, synchronised)  stage B {stage_b:7.3f} ms")
