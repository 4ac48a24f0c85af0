"""parallel.ShardedConnectivity on seed-based connectivity: every rank builds it from ITS share of the trials, sums its seed record
in one pass over its spectra, the records are added over the ranks and every rank runs the small epilogue with the observation
count of the whole job; every rank must get what one process gets from all the trials.  Run under torch.distributed.run;
SC_BENCH_BACKEND=gloo lets all ranks share one GPU (debug / CI on a 1-GPU box)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spectral_connectivity_amd import _lib, parallel  # noqa: E402

MEASURES = tuple(_lib.SEED_MEASURES)
# the bounds of tests/test_gpu_seed_connectivity.py: |a - b| <= tol (|b| + max |b|)
BOUNDS = {np.complex64: dict({m: 1e-5 for m in MEASURES}, phase_locking_value=3e-5, pairwise_phase_consistency=3e-5,
                             debiased_squared_phase_lag_index=1e-4, debiased_squared_weighted_phase_lag_index=1e-4),
          np.complex128: {m: 1e-9 for m in MEASURES}}


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
    rng = np.random.default_rng(21)
    T, R, C = 384, 5, 9                                       # 5 trials: unequal shards (3 + 2 on two ranks)
    x = np.empty((T + 3 * C, R, C))                           # channel j is channel j - 1 delayed by 3 samples plus noise
    x[:, :, 0] = rng.standard_normal((T + 3 * C, R))
    for j in range(1, C):
        x[:, :, j] = np.roll(x[:, :, j - 1], 3, axis=0) + 0.7 * rng.standard_normal((T + 3 * C, R))
    x = x[3 * C:]
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=128,
              n_time_samples_per_step=128)
    seeds, targets = [8, 2], [0, 2, 7, 8, 3]
    lo, hi = parallel.shard_bounds(R, world, rank)
    if world == 2:
        assert (lo, hi) == ((0, 3), (3, 5))[rank], (lo, hi)
    for dtype in (np.complex64, np.complex128):
        for expectation_type in ("trials_tapers", "time_trials_tapers", "trials"):
            mine = parallel.ShardedConnectivity.from_multitaper(sc.Multitaper(x[:, lo:hi], **kw), expectation_type=expectation_type,
                                                                dtype=dtype)
            whole = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), expectation_type=expectation_type, dtype=dtype)
            for tg in (targets, None):
                a, b = mine.seed_connectivity(seeds, tg, MEASURES), whole.seed_connectivity(seeds, tg, MEASURES)
                assert list(a.values) == list(b.values) == list(MEASURES)
                assert np.array_equal(a.targets, b.targets) and np.array_equal(a.seeds, b.seeds)
                for m in MEASURES:
                    got, want = a.values[m], b.values[m]
                    assert got.shape == want.shape and got.dtype == want.dtype, (m, got.shape, want.shape, got.dtype, want.dtype)
                    assert np.array_equal(np.isnan(got), np.isnan(want)), m
                    ok = np.isfinite(want)
                    assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)]), m
                    err = (np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]) + np.abs(want[ok]).max(), 1e-300)).max()
                    if rank == 0:
                        print(f"FIGURE sharded {np.dtype(dtype)} | {expectation_type} | {m} | {err:.3e}", flush=True)
                    assert err <= BOUNDS[dtype][m], f"{expectation_type} {m} ({np.dtype(dtype)}): {err:.3e}"
    dist.barrier()
    if rank == 0:
        print("sharded seed connectivity OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
