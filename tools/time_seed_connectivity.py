"""Device time of Connectivity.seed_connectivity (seed_accumulate_kernel + seed_measure_kernel of sc_seed.hip) beside the all-pairs
coherence_magnitude() + weighted_phase_lag_index() of the same series, both engines.

    python tools/time_seed_connectivity.py               # 306 signals + 2 seeds and 128 signals + 4 seeds at 1000 trials x 7 tapers x
                                                         # 7 windows x 129 bins, then 1024 signals x 100 trials with 16 seeds
    python tools/time_seed_connectivity.py C:S:R ...     # other shapes: signals in all, seeds (the last S signals), trials

Times are the library's own brackets (sc_timing: two events on the stream around the launches of an entry point), summed over the
entry points of a call, best of the repetitions after one that warms up; the spectra are resident before either side is timed (the
seed call reads complex64 / complex128 spectra, the all-pairs methods of the float32 engine the format their first request picks).
"read" is the bytes of spectra the accumulate kernel walks once, over its own time.  The result goes to
profiles/seed_connectivity_time.txt as well (--out PATH for another file)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc      # noqa: E402
from spectral_connectivity_amd import _lib   # noqa: E402

TWO = ("coherence_magnitude", "weighted_phase_lag_index")
TEN = tuple(_lib.SEED_MEASURES)
W, L = 7, 256
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def library_ms(fn, reps=3):
    """{bracket name: best ms} of the library's timers around ``fn`` (one call to warm up first)."""
    best = {}
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        _lib.timing_enable(True)
        _lib.last_timing()
        fn()
        torch.cuda.synchronize()
        once = {}
        for name, ms in _lib.last_timing():
            once[name] = once.get(name, 0.0) + ms
        _lib.timing_enable(False)
        if rep and (not best or sum(once.values()) < sum(best.values())):
            best = once
    return best


def series(C, R):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((W * L, R, C), dtype=np.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    return x


def case(x, n_seeds, dtype):
    C, R = x.shape[2], x.shape[1]
    seeds = list(range(C - n_seeds, C))
    kw = dict(sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L, n_time_samples_per_step=L)
    engine_name = "float32" if dtype == np.complex64 else "float64"
    c = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), dtype=dtype)
    sp = c._device()                            # complex64 / complex128 spectra, resident
    n_bytes = sp.F * sp.W * sp.R * sp.K * sp.C * (16 if sp.f64 else 8)
    res = {}
    for tag, names in (("coherence", TWO[:1]), ("coherence + wPLI", TWO), ("all ten", TEN)):
        res[tag] = library_ms(lambda: c.seed_connectivity(seeds, measures=names))
    seed_two = c.seed_connectivity(seeds, measures=TWO).values
    del c, sp
    torch.cuda.empty_cache()
    # the all-pairs methods on a SECOND object from the same series, not on the one above: their first request picks the device format
    # of the spectra (the planes format on the float32 engine), which is their fastest route; both measures share one stage B
    full = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), dtype=dtype)
    full._prepare(TWO)

    def all_pairs():
        full._accum_cache.clear()
        full._prepare(TWO)
        return full.coherence_magnitude(), full.weighted_phase_lag_index()

    ref = library_ms(all_pairs, reps=2)
    ref = {k: v for k, v in ref.items() if not k.startswith("mtfft")}
    coh, wpli = all_pairs()
    worst = max(np.nanmax(np.abs(seed_two[TWO[0]] - coh[..., seeds, :])), np.nanmax(np.abs(seed_two[TWO[1]] - wpli[..., seeds, :])))
    del full
    torch.cuda.empty_cache()
    t = {k: sum(v.values()) for k, v in res.items()}
    acc = res["coherence + wPLI"]["seed_accumulate"]
    say(f"{engine_name} engine | {C} signals, {n_seeds} seeds, {R} trials x 7 tapers x {W} windows x {L // 2 + 1} bins "
        f"({n_bytes / 1e9:.2f} GB of spectra)")
    for tag in res:
        a = res[tag]["seed_accumulate"]
        say(f"    seed {tag:<16} {t[tag]:9.3f} ms  (accumulate {a:.3f}, epilogue {res[tag]['seed_measure']:.3f}; read "
            f"{n_bytes / a / 1e9:.2f} TB/s = {100 * n_bytes / a / 1e9 / 6.0:.0f} % of the 6.0 TB/s in-order sweep)")
    say(f"    all pairs coherence + wPLI {sum(ref.values()):9.3f} ms  ({', '.join(f'{k} {v:.3f}' for k, v in ref.items())})")
    say(f"    seed / all pairs {t['coherence + wPLI'] / sum(ref.values()):.3f}   accumulate alone {acc:.3f} ms   "
        f"max |seed - all pairs| {worst:.1e}   {'OK' if t['coherence + wPLI'] < sum(ref.values()) else 'SLOWER THAN ALL PAIRS'}")
    return t["coherence + wPLI"] < sum(ref.values())


def main():
    shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:] if not a.startswith("--") and ":" in a]
    shapes = shapes or [(308, 2, 1000), (132, 4, 1000), (1024, 16, 100)]
    say("# tools/time_seed_connectivity.py (expectation_type trials_tapers: 7 kept windows x 129 bins, 7 tapers x the trials observations each)")
    ok = True
    for C, S, R in shapes:
        x = series(C, R)
        for dtype in (np.complex64, np.complex128):
            ok = case(x, S, dtype) and ok
        del x
    say("every shape: the seed call for coherence + wPLI takes less device time than the all-pairs methods" if ok else
        "AT LEAST ONE SHAPE: the seed call is slower than the all-pairs methods")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "seed_connectivity_time.txt")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
