"""Accuracy of the global-coherence eigensolvers (sc_global_coherence_f64) on the hand-built matrices of
tests/global_coherence_ref.py: the four ratios of global_coherence_ref.check per case of tests/test_gpu_global_coherence.py (a).

    python tools/global_coherence_accuracy.py --cpu > profiles/global_coherence_accuracy.txt      # anywhere: sets the bars
    python tools/global_coherence_accuracy.py >> profiles/global_coherence_accuracy.txt           # on an MI355X: informational

--cpu: numpy.linalg.eigh in float64 over every case, every eigenpair; the bars K_VALUES, K_RESIDUAL and K_GRAM of the suite are
8 x the worst ratio of the whole list, rounded up to a power of two (the last line).  Without it: the device's ratios per signal
count (max_rank = n_signals largest first, and min(n_signals, 5) smallest first).  The device rows change no bar.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np                                 # noqa: E402

import global_coherence_ref as gref                # noqa: E402

CHECKS = ("values", "residual", "gram", "phase")


def row(name, C, r):
    return f"{name:>8} {C:>4} " + " ".join(f"{r[k]:>9.2f}" for k in CHECKS)


def header(what):
    print(what)
    print(f"{'case':>13} " + " ".join(f"{k:>9}" for k in CHECKS))


def cpu():
    import test_global_coherence_ref as tref
    header("global coherence on hand-built matrices, numpy.linalg.eigh (float64, NumPy " + np.__version__ + "): worst ratio over the matrices "
           "of the case, every eigenpair\nvalues, residual: / (2^-52 ||A||_2); Gram, phase: / 2^-52")
    worst = dict.fromkeys(CHECKS, 0.0)
    for C in gref.SIZES:
        for family in gref.FAMILIES:
            r = tref.numpy_ratios(family, C)
            print(row(family, C, r), flush=True)
            worst = {k: max(worst[k], r[k]) for k in CHECKS}
    print(f"{'max':>13} " + " ".join(f"{worst[k]:>9.2f}" for k in CHECKS))
    ks = {}
    for k in CHECKS[:3]:
        ks[k] = 1.0
        while ks[k] < 8.0 * worst[k]:
            ks[k] *= 2.0
    print(f"K = 8 x the NumPy maximum, rounded up to a power of two: values {ks['values']:g}, residual {ks['residual']:g}, Gram {ks['gram']:g}")
    committed = (gref.K_VALUES, gref.K_RESIDUAL, gref.K_GRAM)
    if committed != (ks["values"], ks["residual"], ks["gram"]):
        print(f"!! tests/global_coherence_ref.py holds {committed}: update it", file=sys.stderr)
        return 1
    return 0


def device():
    import torch

    import test_gpu_global_coherence as tg
    header(f"\ndevice: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); float64 records; per case "
           "max_rank = n_signals largest first and min(n_signals, 5) smallest first (informational: these rows set no bar)")
    above = []
    for C in gref.SIZES:
        for family in gref.FAMILIES:
            r = {}
            for max_rank, ascending in ((C, False), (min(C, 5), True)):
                for k, v in tg.device_ratios(family, C, max_rank, ascending).items():
                    r[k] = max(v, r.get(k, 0.0))
            print(row(family, C, r), flush=True)
            above += [(family, C, k, v) for k, v in gref.over_the_bars(r, tg.bars_of(family, C)).items()]
    print("device ratios above a bar: " + ("none" if not above else "; ".join(f"{f} {c} {k} {v:.1f}" for f, c, k, v in above)))
    return 0


if __name__ == "__main__":
    sys.exit(cpu() if "--cpu" in sys.argv[1:] else device())
