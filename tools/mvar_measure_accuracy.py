"""Accuracy of the MVAR measure kernels (sc_mvar_measure_f64) on the hand-built factors of tests/mvar_measures_ref.py: per case of
tests/test_gpu_mvar_measures.py (a) and quantity the largest |got - ref| / (2^-52 max |ref|), maxima per window, for the device
and -- up to 132 signals, where the reference is the extended-precision evaluation -- for the float64 NumPy evaluation of the
same case on the CPU.  The table the bounds K_q of that test are taken from (profiles/mvar_measure_accuracy.txt).

    python tools/mvar_measure_accuracy.py > profiles/mvar_measure_accuracy.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mvar_measures_ref as mref            # noqa: E402
import test_gpu_mvar_measures as tgm        # noqa: E402

SHORT = dict(zip(mref.QUANTITIES, ("DTF", "DC", "PDC", "gPDC", "dDTF", "H", "A", "Sigma")))
CLASSES = [("<= 48", 1, 48), ("49-64", 49, 64), ("65-96", 65, 96), ("97-128", 97, 128), ("129-256", 129, 256), ("257-512", 257, 512)]


def cell(dev, ref):
    return f"{dev:6.2f}|{ref:5.2f}" if ref is not None else f"{dev:6.2f}|  -  "


def main():
    import torch
    print("MVAR measures from hand-built factors: max |got - ref| / (2^-52 max |ref|), maxima per window; every cell device|NumPy float64")
    print(f"device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); reference: np.longdouble up to "
          f"{mref.EXTENDED_MAX} signals, NumPy float64 beyond (no NumPy column there); shapes: tests/test_gpu_mvar_measures.py shape_of")
    print(f"{'case':>15} " + " ".join(f"{SHORT[q]:>12}" for q in mref.QUANTITIES))
    by_class = {c[0]: {} for c in CLASSES}
    total, total_np, findings = {}, {}, []
    for C in tgm.SIZES:
        for kind in tgm.KINDS:
            dev, ref = tgm.accuracy_row(kind, C)
            print(f"{kind:>10} {C:>4} " + " ".join(cell(dev[q], ref[q] if ref else None) for q in mref.QUANTITIES), flush=True)
            name = next(c[0] for c in CLASSES if c[1] <= C <= c[2])
            for q in mref.QUANTITIES:
                d, n = by_class[name].get(q, (0.0, None))
                by_class[name][q] = (max(d, dev[q]), max(n or 0.0, ref[q]) if ref else n)
                total[q] = max(total.get(q, 0.0), dev[q])
                total_np[q] = max(total_np.get(q, 0.0), ref[q] if ref else 0.0)
                if ref and dev[q] > 64.0 * max(ref[q], 1.0):
                    findings.append((kind, C, q, dev[q], ref[q]))
    print("\nper size class (signals), device|NumPy float64")
    for name, *_ in CLASSES:
        print(f"{name:>15} " + " ".join(cell(*by_class[name][q]) for q in mref.QUANTITIES))
    print(f"{'max':>15} " + " ".join(cell(total[q], total_np[q]) for q in mref.QUANTITIES))
    ks = {}
    for q in mref.QUANTITIES:
        k = 1.0
        while k < 4.0 * total[q]:
            k *= 2.0
        ks[q] = k
    print("K = 4 x the device maximum, rounded up to a power of two: " + ", ".join(f"{SHORT[q]} {ks[q]:g}" for q in mref.QUANTITIES))
    print("device ratios above 64 x the NumPy ratio of the same case: " +
          ("none" if not findings else "; ".join(f"{k} {c} {SHORT[q]} {d:.1f} against {n:.1f}" for k, c, q, d, n in findings)))


if __name__ == "__main__":
    main()
