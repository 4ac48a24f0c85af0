"""parallel.ShardedConnectivity on linear_dependence / lagged_coherence: every rank builds it from ITS share of the trials, the
bins are split over the ranks and gathered; every rank must get what one process gets from all the trials.  Run under
torch.distributed.run; SC_BENCH_BACKEND=gloo lets all ranks share one GPU (debug / CI on a 1-GPU box)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spectral_connectivity_amd import parallel  # noqa: E402


def close(a, b, tol, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]).max()
    assert err <= tol * max(1.0, np.abs(b[ok]).max()), f"{what}: {err}"


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
    T, R, C = 512, 9, 14                                      # 9 trials: unequal shards
    e = rng.standard_normal((T, R, C))
    x = np.zeros_like(e)
    for t in range(2, T):
        x[t] = 0.4 * x[t - 1] - 0.2 * x[t - 2] + e[t]
        x[t, :, 1:] += 0.3 * x[t - 2, :, :-1]
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=128,
              n_time_samples_per_step=128)
    labels = np.array(["c", "a", "b"] * 4 + ["a", "b"])
    lo, hi = parallel.shard_bounds(R, world, rank)
    for dtype, tol in ((np.complex64, 1e-4), (np.complex128, 1e-9)):
        mine = parallel.ShardedConnectivity.from_multitaper(sc.Multitaper(x[:, lo:hi], **kw), dtype=dtype)
        whole = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), dtype=dtype)
        a, b = mine.linear_dependence(labels), whole.linear_dependence(labels)
        assert list(a.labels) == list(b.labels) == ["a", "b", "c"] and b.total.shape == (4, 65, 3, 3)
        for name in ("total", "instantaneous", "lagged"):
            close(getattr(a, name), getattr(b, name), tol, f"{name} ({np.dtype(dtype)})")
        assert np.nanmax(b.lagged) > 0.05
        a, b = mine.linear_dependence(), whole.linear_dependence()           # the pairwise kernel
        assert b.lagged.shape == (4, 65, C, C) and np.array_equal(a.labels, np.arange(C))
        for name in ("total", "instantaneous", "lagged"):
            close(getattr(a, name), getattr(b, name), tol, f"pairwise {name} ({np.dtype(dtype)})")
        close(mine.lagged_coherence(), whole.lagged_coherence(), tol, f"lagged_coherence ({np.dtype(dtype)})")
    dist.barrier()
    if rank == 0:
        print("sharded linear dependence OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
