"""Device time of Connectivity.seed_jackknife (sjk_kernel of sc_seed_jackknife.hip: a totals pass and a jackknife pass) beside the
all-pairs jackknife of the same measures and beside seed_connectivity of the same measures, both engines.

    python tools/time_seed_jackknife.py               # 306 signals + 2 seeds and 128 signals + 4 seeds at 1000 trials x 7 tapers x
                                                      # 7 windows x 129 bins, then 1024 signals x 100 trials with 16 seeds
    python tools/time_seed_jackknife.py C:S:R ...     # other shapes: signals in all, seeds (the last S signals), trials

Times are the library's own brackets (sc_timing: two events on the stream around the launches of an entry point), summed over the
entry points of a call, best of three after one call that warms up; the spectra are resident before anything is timed.  The seed
side is the public call, its cached totals dropped before every repetition, so both passes run.  The all-pairs side -- code this
tool's subject does not touch -- runs on a second object from the same series through the drivers of Connectivity.jackknife
(_stage_d.jackknife against the cached CSM record, whose accumulation is NOT counted; _stage_d.jackknife_phase_totals and
jackknife_phase), its [bin][C][C] outputs left on the device; it is run where the three such arrays per measure fit comfortably
(up to ALL_PAIRS_MAX_SIGNALS signals).  over="observations" is timed at OBS_TRIALS trials (every taper of every trial is a unit, and
the statistic is evaluated after every row).  With two seeds the three splits of a workgroup's four waves are timed too
(the diagnostic switch SC_SEED_JACKKNIFE_CHUNK).  The result goes to profiles/seed_jackknife_time.txt as well (--out PATH for another file), line by line."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc                    # noqa: E402
from spectral_connectivity_amd import _lib, _stage_d     # noqa: E402

SIX = tuple(_lib.SEED_JACKKNIFE_MEASURES)
SETS = (("coherence", SIX[:1]), ("coherence + wPLI", (SIX[0], SIX[3])), ("all six", SIX))
W, L = 7, 256
ALL_PAIRS_MAX_SIGNALS = 512
OBS_TRIALS = 100
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "seed_jackknife_time.txt")
KW = dict(sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L, n_time_samples_per_step=L)


def say(line, first=False):
    print(line, flush=True)
    with open(OUT, "w" if first else "a") as f:
        f.write(line + "\n")


def library_ms(fn, reps=3, before=None):
    """{bracket name: best ms} of the library's timers around ``fn`` (one call to warm up first); ``before`` runs untimed."""
    best = {}
    for rep in range(reps + 1):
        if before:
            before()
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


def drop_totals(c, tag):
    for k in [k for k in c._accum_cache if isinstance(k, tuple) and k[0] == tag]:
        del c._accum_cache[k]


def all_pairs(full, names, over):
    """The device work of full.jackknife(names, over), outputs left on the device: {family: flat output}."""
    old, new = _lib.jackknife_split(names)
    sp, out = full._device(), {}
    if old:
        _, mask, over_id, n_units = _lib.jackknife_request(old, over, full.expectation_type, full._jackknife_trials(), full.n_observations)
        accum, _, _ = full._csm_records("interaction", two_sided=False)
        out["first"], _ = _stage_d.jackknife(full._memory(accum), sp, full.expectation_type, accum, _lib.PLANE_CSM, mask, over_id, n_units,
                                             n_freq=full._n_freq)
    if new:
        _, mask, over_id, n_units, planes = _lib.jackknife_phase_request(new, over, full.expectation_type, full._jackknife_trials(),
                                                                         full.n_observations)
        mem = full._memory(sp.X)
        total, _ = _stage_d.jackknife_phase_totals(mem, sp, full.expectation_type, planes, over_id, n_freq=full._n_freq)
        out["phase"], _ = _stage_d.jackknife_phase(mem, sp, full.expectation_type, total, planes, mask, over_id, n_units, n_freq=full._n_freq)
    return out


def fmt(best):
    return ", ".join(f"{k} {v:.3f}" for k, v in best.items())


def case(x, n_seeds, dtype):
    C, R = x.shape[2], x.shape[1]
    seeds = list(range(C - n_seeds, C))
    engine_name = "float32" if dtype == np.complex64 else "float64"
    c = sc.Connectivity.from_multitaper(sc.Multitaper(x, **KW), dtype=dtype)
    sp = c._device()                            # complex64 / complex128 spectra, resident
    n_bytes = sp.F * sp.W * sp.R * sp.K * sp.C * (16 if sp.f64 else 8)
    say(f"{engine_name} engine | {C} signals, {n_seeds} seeds, {R} trials x 7 tapers x {W} windows x {L // 2 + 1} bins "
        f"({n_bytes / 1e9:.2f} GB of spectra), over trials: {R} units of 7 rows")
    seed_ms, floor_ms = {}, {}
    for tag, names in SETS:
        seed_ms[tag] = library_ms(lambda: c.seed_jackknife(seeds, measures=names), before=lambda: drop_totals(c, "seed_jackknife"))
        floor_ms[tag] = library_ms(lambda: c.seed_connectivity(seeds, measures=names))
    if n_seeds == 2:
        for width in ("4", "2", "1"):
            _lib.set_debug_env("SC_SEED_JACKKNIFE_CHUNK", width)
            t = library_ms(lambda: c.seed_jackknife(seeds, measures=SIX), before=lambda: drop_totals(c, "seed_jackknife"))
            say(f"    all six with {width} seed(s) x {256 // int(width)} targets per workgroup: {sum(t.values()):9.3f} ms  ({fmt(t)})")
        _lib.set_debug_env("SC_SEED_JACKKNIFE_CHUNK", None)
    coherence = c.seed_jackknife(seeds, measures=SIX[:1]).results[SIX[0]].estimate
    del c, sp
    torch.cuda.empty_cache()
    ok, pairs_ms = True, {}
    if C <= ALL_PAIRS_MAX_SIGNALS:
        full = sc.Connectivity.from_multitaper(sc.Multitaper(x, **KW), dtype=dtype)
        full._device()
        for tag, names in SETS:
            pairs_ms[tag] = library_ms(lambda: all_pairs(full, names, "trials"), reps=2)
        theta = all_pairs(full, SIX[:1], "trials")["first"]
        n_bins = theta.numel() // (3 * C * C)
        theta = theta[:n_bins * C * C].view(n_bins, C, C)[:, seeds, :].cpu().numpy().reshape(coherence.shape)
        worst = np.nanmax(np.abs(coherence - theta))
        del full, theta
        torch.cuda.empty_cache()
    for tag, _ in SETS:
        s, f = sum(seed_ms[tag].values()), sum(floor_ms[tag].values())
        walk = seed_ms[tag]["seed_jackknife"]
        say(f"    seed jackknife {tag:<16} {s:9.3f} ms  (totals pass {seed_ms[tag]['seed_jackknife_totals']:.3f}, jackknife pass "
            f"{walk:.3f}: {n_bytes / walk / 1e9:.2f} TB/s of spectra)   seed_connectivity {f:.3f} ms: x {s / f:.1f}")
        if pairs_ms:
            p = sum(pairs_ms[tag].values())
            ok = ok and s < p
            say(f"    all-pairs jackknife {tag:<11} {p:9.3f} ms  ({fmt(pairs_ms[tag])})   seed / all pairs {s / p:.4f}   "
                f"{'OK' if s < p else 'SLOWER THAN ALL PAIRS'}")
    if pairs_ms:
        say(f"    work ratio S T : C^2 / 2 = 1 : {C * C / 2 / (n_seeds * C):.1f}   max |seed - all pairs| of the coherence estimate {worst:.1e}")
    else:
        say(f"    all-pairs jackknife not run: its three [bin][C][C] float64 arrays are {3 * 903 * C * C * 8 / 1e9:.1f} GB per measure")
    return ok


def observations(x, n_seeds, dtype):
    C, R = x.shape[2], x.shape[1]
    seeds = list(range(C - n_seeds, C))
    c = sc.Connectivity.from_multitaper(sc.Multitaper(x, **KW), dtype=dtype)
    c._device()
    for tag, names in SETS:
        t = library_ms(lambda: c.seed_jackknife(seeds, measures=names, over="observations"), before=lambda: drop_totals(c, "seed_jackknife"))
        say(f"    over observations, {R} trials = {7 * R} units of 1 row, {'float32' if dtype == np.complex64 else 'float64'} engine, "
            f"{tag:<16} {sum(t.values()):9.3f} ms  ({fmt(t)})")
    del c
    torch.cuda.empty_cache()


def main():
    shapes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:] if not a.startswith("--") and ":" in a]
    shapes = shapes or [(308, 2, 1000), (132, 4, 1000), (1024, 16, 100)]
    say("# tools/time_seed_jackknife.py (expectation_type trials_tapers: 7 kept windows x 129 bins = 903 bin records)", first=True)
    ok = True
    for C, S, R in shapes:
        x = series(C, R)
        for dtype in (np.complex64, np.complex128):
            ok = case(x, S, dtype) and ok
        xo = x[:, :OBS_TRIALS]
        for dtype in (np.complex64, np.complex128):
            observations(xo, S, dtype)
        del x, xo
    say("every shape where the all-pairs jackknife ran: the seed call takes less device time" if ok else
        "AT LEAST ONE SHAPE: the seed call is slower than the all-pairs jackknife")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
