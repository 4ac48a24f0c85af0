"""parallel.ShardedConnectivity on Connectivity.seed_jackknife: every rank builds it from ITS share of the trials, sums its totals
record, walks its own delete units against the all-reduced record and the stacked partial sums are added over the ranks; every rank
must get what one process gets from all the trials.  Run under torch.distributed.run; SC_BENCH_BACKEND=gloo lets all ranks share
one GPU (debug / CI on a 1-GPU box)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spectral_connectivity_amd import _lib, parallel  # noqa: E402

MEASURES = tuple(_lib.SEED_JACKKNIFE_MEASURES)
# the bounds of tests/test_gpu_seed_jackknife.py
BOUNDS = {np.complex64: {"estimate": 2e-6, "bias_corrected": 4e-6, "standard_error": 1e-3},
          np.complex128: {"estimate": 1e-9, "bias_corrected": 1e-9, "standard_error": 1e-9}}


def main():
    import spectral_connectivity_amd as sc
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    backend = os.environ.get("SC_BENCH_BACKEND", "nccl")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if backend != "nccl":
        local %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    rng = np.random.default_rng(12)
    T, R, C = 512, 7, 7                                       # 7 trials: unequal shards (4 + 3 on two ranks)
    x = np.empty((T + 3 * C, R, C))                           # channel j is channel j - 1 delayed by 3 samples plus noise
    x[:, :, 0] = rng.standard_normal((T + 3 * C, R))
    for j in range(1, C):
        x[:, :, j] = np.roll(x[:, :, j - 1], 3, axis=0) + 0.7 * rng.standard_normal((T + 3 * C, R))
    x = x[3 * C:]
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=128,
              n_time_samples_per_step=128)
    seeds, targets = [6, 2], [0, 6, 5, 1, 3]
    lo, hi = parallel.shard_bounds(R, world, rank)
    if world == 2:
        assert (lo, hi) == ((0, 4), (4, 7))[rank], (lo, hi)
    for dtype in (np.complex64, np.complex128):
        for expectation_type, over in (("trials_tapers", "trials"), ("time_trials_tapers", "trials"), ("trials_tapers", "observations")):
            mine = parallel.ShardedConnectivity.from_multitaper(sc.Multitaper(x[:, lo:hi], **kw), expectation_type=expectation_type,
                                                                dtype=dtype)
            whole = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), expectation_type=expectation_type, dtype=dtype)
            a, b = mine.seed_jackknife(seeds, targets, MEASURES, over=over), whole.seed_jackknife(seeds, targets, MEASURES, over=over)
            assert np.array_equal(a.seeds, b.seeds) and np.array_equal(a.targets, b.targets)
            a, b = a.results, b.results
            assert list(a) == list(b) == list(MEASURES)
            for m in MEASURES:
                assert a[m].n_units == b[m].n_units == (R if over == "trials" else R * 3), (m, a[m].n_units)
                # what the sum form can resolve in the square of a standard error: tools/check_sharded_phase_lag_jackknife.py
                q = 1e-15 * (b[m].bias_corrected - b[m].estimate) ** 2
                for o, tol in BOUNDS[dtype].items():
                    got, want = getattr(a[m], o), getattr(b[m], o)
                    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (m, o)
                    ok = ~np.isnan(want)
                    diff = np.abs(got - want)
                    if o == "standard_error":
                        upper, lower = np.sqrt(want ** 2 + q), np.sqrt(np.maximum(want ** 2 - q, 0.0))
                        diff = np.maximum(np.maximum(got - upper, lower - got), 0.0)
                        assert np.all(diff[ok & (want == 0)] == 0), (m, o)
                        ok &= want != 0
                    scale = np.abs(want[ok]) if o == "standard_error" else 1 + np.abs(want[ok])
                    err = (diff[ok] / scale).max()
                    if rank == 0:
                        print(f"FIGURE sharded {np.dtype(dtype)} | {expectation_type} over {over} | {m} | {o} | {err:.3e}", flush=True)
                    assert err <= tol, f"{expectation_type} over {over} {m} {o} ({np.dtype(dtype)}): {err:.3e}"
    dist.barrier()
    if rank == 0:
        print("sharded seed jackknife OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
