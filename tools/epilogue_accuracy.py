"""Accuracy of the one-launch measures epilogue (measure_tile_multi_kernel) on hand-built records against the extended-precision
reference of tests/epilogue_ref.py: per channel count and measure the largest |got - ref| / (2^-52 cond) over float and double
records, wide output -- the table the bound K of tests/test_gpu_epilogue.py is taken from (profiles/epilogue_accuracy.txt).

    python tools/epilogue_accuracy.py > profiles/epilogue_accuracy.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import epilogue_ref as eref                 # noqa: E402
import test_gpu_epilogue as tge             # noqa: E402

SHORT = {"coherence_magnitude": "coh", "coherence_phase": "phase", "imaginary_coherence": "imcoh", "phase_locking_value": "plv",
         "phase_lag_index": "pli", "weighted_phase_lag_index": "wpli", "debiased_squared_phase_lag_index": "dpli2",
         "debiased_squared_weighted_phase_lag_index": "dwpli2", "pairwise_phase_consistency": "ppc"}


def main():
    import torch
    print("measures epilogue, one-launch kernel, wide output: max |got - ref| / (2^-52 cond) over 3 bins, float and double records")
    print(f"device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); reference: np.longdouble (tests/epilogue_ref.py), n_obs = {tge.N_OBS}")
    print(f"{'C':>5} " + " ".join(f"{SHORT[m]:>7}" for m in eref.REAL_MEASURES))
    total = {}
    for C in tge.CHANNELS:
        row = tge.accuracy_table([C])
        print(f"{C:>5} " + " ".join(f"{row[m]:7.2f}" for m in eref.REAL_MEASURES))
        for m, v in row.items():
            total[m] = max(total.get(m, 0.0), v)
    print(f"{'max':>5} " + " ".join(f"{total[m]:7.2f}" for m in eref.REAL_MEASURES))
    worst = max(total.values())
    k = 1.0
    while k < 4.0 * worst:
        k *= 2.0
    print(f"overall maximum {worst:.2f} ({max(total, key=total.get)}); K = 4 x that, rounded up to a power of two = {k:g}")


if __name__ == "__main__":
    main()
