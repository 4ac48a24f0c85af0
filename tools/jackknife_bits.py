"""The bits of the three jackknife kernels of sc_jackknife.hip: one SHA-256 per (case, engine, entry point, mask or planes) of what
engine.jackknife, engine.jackknife_phase and engine.jackknife_phase_totals return -- the raw theta(S), sum d, sum d^2 arrays and the
totals record, before any host finishing -- on seeded spectra.  Two builds of the library compute the same numbers exactly when
their listings are equal line for line.

    python tools/jackknife_bits.py [--out PATH]

The cases are the smallest that reach every path of the walk (jk_place, jk_walk): tile edges, a unit longer than one staging, units
that straddle stagings, unit splits and their fold, the per-row decode of over = observations, a unit range inside the units."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spectral_connectivity_amd import _lib, engine      # noqa: E402

TRIALS, OBSERVATIONS = _lib.JACKKNIFE_OVER["trials"], _lib.JACKKNIFE_OVER["observations"]
PHASE_PLANES_ALL = _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ | _lib.PLANE_SIGN_IM
# name: (F, W, R, K, C, expectation_type, over, unit_range)
CASES = {
    "C=3 (one diagonal tile pair)": (3, 1, 20, 2, 3, "trials_tapers", TRIALS, None),
    "C=17 (a tile edge inside a 32-tile)": (3, 1, 20, 2, 17, "trials_tapers", TRIALS, None),
    "C=33 (two tiles: an off-diagonal pair, a mostly empty tile)": (3, 1, 20, 2, 33, "trials_tapers", TRIALS, None),
    "3 trials, W x K = 5 x 7 (g = 35 rows > one staging)": (4, 5, 3, 7, 5, "time_trials_tapers", TRIALS, None),
    "50 trials, W x K = 3 x 2 (g = 6 straddles stagings, three splits)": (4, 3, 50, 2, 6, "time_trials_tapers", TRIALS, None),
    "1000 trials x 7 tapers, C=16 (many splits and the fold)": (3, 1, 1000, 7, 16, "trials_tapers", TRIALS, None),
    "over observations, W, R, K = 3, 5, 2 (the per-row decode)": (5, 3, 5, 2, 6, "time_trials_tapers", OBSERVATIONS, None),
    "units 5 .. 37 of 50 (unit_begin > 0, n_units_total = 50)": (4, 3, 50, 2, 6, "time_trials_tapers", TRIALS, (5, 37)),
}


def spectra(F, W, R, K, C, dtype):
    """Seeded [F][W][R][K][C] coefficients, neighbouring channels correlated; complex64 rows get the float32 engine's zero pad channel."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((F, W, R, K, C)) + 1j * rng.standard_normal((F, W, R, K, C))
    x[..., 1:] += 0.6 * x[..., :-1]
    C_alloc = C + (C & 1) if dtype == np.complex64 else C
    X = np.zeros((F, W, R, K, C_alloc), dtype=dtype)
    X[..., :C] = x
    return engine.DeviceSpectra(torch.from_numpy(X).cuda().view(-1), (F, W, R, K, C), (W * R * K * C_alloc, R * K * C_alloc, K * C_alloc, C_alloc),
                                2 * (F - 1), True, C_alloc=C_alloc)


def phase_planes(mask):
    planes = 0
    for name, (bit, _, _) in _lib.JACKKNIFE_PHASE_MEASURES.items():
        if mask & bit:
            planes |= _lib.JACKKNIFE_PHASE_PLANES[name]
    return planes


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    lines = []
    for case, (F, W, R, K, C, expectation_type, over, unit_range) in CASES.items():
        for dtype, name in ((np.complex64, "complex64"), (np.complex128, "complex128")):
            sp = spectra(F, W, R, K, C, dtype)
            n_units = R if over == TRIALS else W * R * K
            kw = dict(n_freq=F, unit_range=unit_range)
            total, _ = engine.accumulate(sp, expectation_type, _lib.PLANE_CSM, n_freq=F)
            for mask in (0x1, 0x2, 0x4, 0x7):
                out, _ = engine.jackknife(sp, expectation_type, total, _lib.PLANE_CSM, mask, over, n_units, **kw)
                lines.append(f"{case} | {name} | jackknife | measures {mask:#x} | {sha(out)}")
            for mask in (0x1, 0x2, 0x4, 0x8, 0xF):
                planes = phase_planes(mask)
                record, _ = engine.jackknife_phase_totals(sp, expectation_type, planes, over, n_freq=F)     # (of all the units)
                out, _ = engine.jackknife_phase(sp, expectation_type, record, planes, mask, over, n_units, **kw)
                lines.append(f"{case} | {name} | jackknife_phase | measures {mask:#x} | {sha(out)}")
            for planes in (_lib.PLANE_SIGN_IM, PHASE_PLANES_ALL):
                record, _ = engine.jackknife_phase_totals(sp, expectation_type, planes, over, **kw)
                lines.append(f"{case} | {name} | jackknife_phase_totals | planes {planes:#x} | {sha(record)}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
