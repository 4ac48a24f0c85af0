"""parallel.ShardedConnectivity on partial and multiple coherence given a chosen set of signals: every rank builds it from ITS share
of the trials, the bins are split over the ranks and gathered; every rank must get what one process gets from all the trials.  Run
under torch.distributed.run; SC_BENCH_BACKEND=gloo lets all ranks share one GPU (debug / CI on a 1-GPU box)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spectral_connectivity_amd import parallel  # noqa: E402


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
    T, R, C = 512, 9, 6                                       # 9 trials: unequal shards
    e = rng.standard_normal((T, R, C))
    x = np.zeros_like(e)
    for t in range(2, T):
        x[t] = 0.4 * x[t - 1] - 0.2 * x[t - 2] + e[t]
        x[t, :, 1:] += 0.3 * x[t - 2, :, :-1]
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=128,
              n_time_samples_per_step=128)
    lo, hi = parallel.shard_bounds(R, world, rank)
    given, signals = [4, 0], [5, 1, 2]
    shapes = {"partial_coherency": (4, 65, 3, 3), "partial_coherence_magnitude": (4, 65, 3, 3), "multiple_coherence_magnitude": (4, 65, 3)}
    for dtype, tol in ((np.complex64, 1e-4), (np.complex128, 1e-9)):
        mine = parallel.ShardedConnectivity.from_multitaper(sc.Multitaper(x[:, lo:hi], **kw), dtype=dtype)
        whole = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), dtype=dtype)
        for name, shape in shapes.items():
            a, b = getattr(mine, name)(given=given, signals=signals), getattr(whole, name)(given=given, signals=signals)
            assert a.shape == b.shape == shape and a.dtype == b.dtype, (name, a.shape, a.dtype)
            assert np.array_equal(np.isnan(a), np.isnan(b)), name
            ok = ~np.isnan(b)
            err = np.abs(a[ok] - b[ok]).max()
            assert err <= tol, f"{name} ({np.dtype(dtype)}): {err}"
            assert np.abs(b[ok]).max() > 0.1, name
    dist.barrier()
    if rank == 0:
        print("sharded partial coherence given a set OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
