"""The canonical-coherence vectors (sc_canonical_coherence_vectors_f64) against canonical coherence alone
(sc_canonical_coherence_f64) and against the MIC vectors (sc_imaginary_interaction_vectors_f64) on the same records: library time
of each call (sc_timing brackets, device time between two events on the stream), best of the repetitions after one that warms
up, 7 windows x 513 bins (1024-sample windows), float64 engine.
Usage: python tools/canonical_vectors_time.py [n_groups:group_size ...].  Default 16:16 8:32 4:64 2:128."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc      # noqa: E402
from spectral_connectivity_amd import _lib   # noqa: E402

cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:] if not a.startswith("--")] or [(16, 16), (8, 32), (4, 64), (2, 128)]
W, L = 7, 1024
for n_groups, size in cases:
    C = n_groups * size
    R = max(8, -(-(size + 8) // 7))          # trials x 7 tapers: more observations than the channels of a group
    rng = np.random.default_rng(9)
    x = rng.standard_normal((W * L, R, C)).astype(np.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    labels = np.arange(C) // size
    m = sc.Multitaper(x, sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    c = sc.Connectivity.from_multitaper(m, expectation_type="trials_tapers")
    c._csm_records("canonical", "trials_tapers", two_sided=False)       # the records of each family, before the timed calls
    c._csm_records("interaction", two_sided=False)
    torch.cuda.synchronize()
    best = {}
    for rep in range(3):
        _lib.timing_enable(True)
        _lib.last_timing()
        cc, _ = c.canonical_coherence(labels)
        mic = c.maximized_imaginary_coherence_vectors(labels)
        out = c.canonical_coherence_vectors(labels)
        torch.cuda.synchronize()
        for k, v in _lib.last_timing():
            if rep > 0:
                best[k] = min(best.get(k, 1e30), v)
        _lib.timing_enable(False)
    canon, micv, vec = best["canonical_coherence"], best["imaginary_interaction_vectors"], best["canonical_coherence_vectors"]
    ok = ~np.isnan(cc)
    print(f"{n_groups} groups x {size} channels, {W} windows x {cc.shape[-3]} bins, {R} trials: canonical coherence {canon:.2f} ms, "
          f"MIC vectors {micv:.2f} ms, canonical vectors {vec:.2f} ms (x {vec / micv:.2f} the MIC vectors, x {vec / canon:.1f} the "
          f"value alone); finite vectors {np.isfinite(out.filters).mean():.2f}, "
          f"max |coherence^2 - canonical_coherence| {np.abs(out.coherence[ok] ** 2 - cc[ok]).max():.1e}", flush=True)
