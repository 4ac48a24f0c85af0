"""parallel.ShardedConnectivity on the canonical-coherence vectors: every rank builds it from ITS share of the trials, the bins are
split over the ranks and gathered (the coherences, filters and patterns with their extra trailing axes); every rank must get what
one process gets from all the trials.  Run under torch.distributed.run; SC_BENCH_BACKEND=gloo lets all ranks share one GPU (debug /
CI on a 1-GPU box)."""
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
    # The two estimates sum the trials in different orders, so their records differ by rounding and a vector by that times its
    # eigenvector amplification (unbounded where two canonical coherences cross): the values, shapes, NaN cells and members are
    # compared everywhere, the vectors where the two sides span the same direction -- which must be nearly everywhere.
    for dtype, tol in ((np.complex64, 1e-4), (np.complex128, 1e-9)):
        mine = parallel.ShardedConnectivity.from_multitaper(sc.Multitaper(x[:, lo:hi], **kw), dtype=dtype)
        whole = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), dtype=dtype)
        a = mine.canonical_coherence_vectors(labels)
        b = whole.canonical_coherence_vectors(labels)
        assert a.coherence.shape == b.coherence.shape == (4, 65, 3, 3) and a.coherences.shape == b.coherences.shape == (4, 65, 3, 3, 5)
        assert a.filters.shape == b.filters.shape == a.patterns.shape == b.patterns.shape == (4, 65, 3, 3, 5), a.filters.shape
        assert a.filters.dtype == a.patterns.dtype == np.complex128
        assert list(a.labels) == list(b.labels) == ["a", "b", "c"]
        assert all(np.array_equal(p, q) for p, q in zip(a.members, b.members)) and [len(m) for m in a.members] == [5, 5, 4]
        for name in ("coherence", "coherences", "filters", "patterns"):
            assert np.array_equal(np.isnan(getattr(a, name)), np.isnan(getattr(b, name))), name
        for name in ("coherence", "coherences"):
            ok = ~np.isnan(getattr(b, name))
            err = np.abs(getattr(a, name)[ok] - getattr(b, name)[ok]).max()
            assert err <= tol, f"{name} ({np.dtype(dtype)}): {err}"
        cc, _ = mine.canonical_coherence(labels)
        ok = ~np.isnan(cc)
        assert np.abs(a.coherence[ok] ** 2 - cc[ok]).max() <= tol
        # every finite entry of this rank's gathered arrays was computed by some rank: every bin holds finite vectors
        assert np.isfinite(a.filters[:, :, 0, 1]).all() and np.isfinite(a.patterns[:, :, 2, 0, :4]).all()
        pa, pb = np.nan_to_num(a.patterns), np.nan_to_num(b.patterns)
        cos = np.abs((np.conj(pa) * pb).sum(-1)) / np.maximum(np.linalg.norm(pa, axis=-1) * np.linalg.norm(pb, axis=-1), 1e-300)
        off = ~np.eye(3, dtype=bool)
        close = cos[..., off] >= 1 - 1e3 * tol
        assert close.mean() >= 0.9, f"patterns ({np.dtype(dtype)}): only {close.mean():.2f} of the pairs agree"
    dist.barrier()
    if rank == 0:
        print("sharded canonical vectors OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
