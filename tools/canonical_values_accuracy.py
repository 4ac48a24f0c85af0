"""Accuracy of the value kernels of canonical coherence and of the imaginary interaction (sc_canonical_coherence_f64,
sc_imaginary_interaction_f64) on the hand-built records of tests/canonical_values_ref.py: the error of rho_1^2, MIC and MIM per case
of tests/test_gpu_canonical_values.py (a) and of the conditioning series (e).

    python tools/canonical_values_accuracy.py --cpu > profiles/canonical_values_accuracy.txt      # anywhere: sets the bars
    python tools/canonical_values_accuracy.py >> profiles/canonical_values_accuracy.txt           # on an MI355X: informational

--cpu: the plain NumPy float64 reference (numpy.linalg.cholesky, two triangular solves, svd) over every case; the bars K_CANONICAL,
K_MIC, K_MIM and K_CONDITIONING of the suite are 8 x the worst ratio of their column, rounded up to a power of two (the last
lines).  Without it: the device's ratios per case, both label orders.  The device rows change no bar.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np                                 # noqa: E402

import canonical_values_ref as vref                # noqa: E402

KINDS = ("canonical", "mic", "mim")


def row(name, sizes, r):
    return f"{name:>8} {sizes[0]:>4} {sizes[1]:>4} " + " ".join(f"{r[k]:>9.2f}" for k in KINDS)


def header(what):
    print(what)
    print(f"{'case':>18} " + " ".join(f"{k:>9}" for k in KINDS))


def table(ratios, conditioning):
    """the rows of (a) and of the conditioning series; returns (worst per kind, worst of the series)"""
    worst = dict.fromkeys(KINDS, 0.0)
    for sizes in vref.PAIR_SIZES:
        for family in vref.FAMILIES:
            r = ratios(family, sizes)
            print(row(family, sizes, r), flush=True)
            worst = {k: max(worst[k], r[k]) for k in KINDS}
    print(f"{'max':>18} " + " ".join(f"{worst[k]:>9.2f}" for k in KINDS))
    print("conditioning series (family exact, gains 2^0 ... 2^(p / 2)): worst of the three values / (2^-52 (kappa_a + kappa_b))")
    worst_c = 0.0
    for sizes in vref.CONDITIONING_SIZES:
        for p in vref.CONDITIONING:
            r = conditioning(sizes, p)
            print(f"{'p = ' + str(p):>8} {sizes[0]:>4} {sizes[1]:>4} {r:>9.3f}", flush=True)
            worst_c = max(worst_c, r)
    print(f"{'max':>18} {worst_c:>9.3f}")
    return worst, worst_c


def cpu():
    header("canonical coherence (rho_1^2), MIC (rho_1) and MIM (sum rho_k^2) on hand-built records, plain NumPy reference (cholesky, two "
           "solves, svd; float64, NumPy " + np.__version__ + "):\nworst error over the bins of the case / 2^-52 (MIM: / (2^-52 min(na, nb)))")
    worst, worst_c = table(vref.numpy_ratios, vref.numpy_conditioning_ratio)
    ks = {k: vref.bar_from(worst[k]) for k in KINDS}
    kc = vref.bar_from(worst_c)
    print(f"K = 8 x the NumPy maximum, rounded up to a power of two: canonical {ks['canonical']:g}, MIC {ks['mic']:g}, MIM {ks['mim']:g}, "
          f"conditioning {kc:g}")
    committed = (vref.K_CANONICAL, vref.K_MIC, vref.K_MIM, vref.K_CONDITIONING)
    if committed != (ks["canonical"], ks["mic"], ks["mim"], kc):
        print(f"!! tests/canonical_values_ref.py holds {committed}: update it", file=sys.stderr)
        return 1
    return 0


def device():
    import torch

    import test_gpu_canonical_values as tg
    header(f"\ndevice: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); float64 records; per case the "
           "worst of both label orders (informational: these rows set no bar)")
    worst, worst_c = table(tg.device_ratios, tg.device_conditioning_ratio)
    above = [f"{k} {worst[k]:.1f}" for k in KINDS if not worst[k] <= vref.BARS[k]]
    if not worst_c <= vref.K_CONDITIONING:
        above.append(f"conditioning {worst_c:.2f}")
    print("device maxima above a bar: " + ("none" if not above else "; ".join(above)))
    return 0


if __name__ == "__main__":
    sys.exit(cpu() if "--cpu" in sys.argv[1:] else device())
