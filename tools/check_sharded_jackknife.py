"""parallel.ShardedConnectivity on the jackknife: every rank builds it from ITS share of the trials, walks its own delete units
against the all-reduced total record and the partial sums are added over the ranks; every rank must get what one process gets from
all the trials.  Run under torch.distributed.run; SC_BENCH_BACKEND=gloo lets all ranks share one GPU (debug / CI on a 1-GPU box)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spectral_connectivity_amd import parallel  # noqa: E402

MEASURES = ("power", "coherence_magnitude", "imaginary_coherence")
# the bounds of tests/test_gpu_jackknife.py
BOUNDS = {np.complex64: {"estimate": 2e-6, "bias_corrected": 8e-5, "standard_error": 1e-3},
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
    T, R, C = 512, 5, 7                                       # 5 trials: unequal shards (3 + 2 on two ranks)
    M = np.eye(C) + 0.4 * rng.standard_normal((C, C))
    x = rng.standard_normal((T, R, C)) @ M.T
    kw = dict(sampling_frequency=200.0, time_halfbandwidth_product=2, n_time_samples_per_window=128,
              n_time_samples_per_step=128)
    lo, hi = parallel.shard_bounds(R, world, rank)
    for dtype in (np.complex64, np.complex128):
        for expectation_type, over in (("trials_tapers", "trials"), ("time_trials_tapers", "trials"), ("trials_tapers", "observations")):
            mine = parallel.ShardedConnectivity.from_multitaper(sc.Multitaper(x[:, lo:hi], **kw), expectation_type=expectation_type,
                                                                dtype=dtype)
            whole = sc.Connectivity.from_multitaper(sc.Multitaper(x, **kw), expectation_type=expectation_type, dtype=dtype)
            a, b = mine.jackknife(MEASURES, over=over), whole.jackknife(MEASURES, over=over)
            for m in MEASURES:
                assert a[m].n_units == b[m].n_units == (R if over == "trials" else R * 3), (m, a[m].n_units)
                for o, tol in BOUNDS[dtype].items():
                    got, want = getattr(a[m], o), getattr(b[m], o)
                    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (m, o)
                    ok = ~np.isnan(want)
                    if o == "standard_error":             # (exactly 0 at the zero and Nyquist bins of the imaginary coherence)
                        assert np.all(got[ok & (want == 0)] == 0), (m, o)
                        ok &= want != 0
                    scale = np.abs(want[ok]) if o == "standard_error" else 1 + np.abs(want[ok])
                    err = (np.abs(got[ok] - want[ok]) / scale).max()
                    if rank == 0:
                        print(f"FIGURE sharded {np.dtype(dtype)} | {expectation_type} over {over} | {m} | {o} | {err:.3e}", flush=True)
                    assert err <= tol, f"{expectation_type} over {over} {m} {o} ({np.dtype(dtype)}): {err:.3e}"
    dist.barrier()
    if rank == 0:
        print("sharded jackknife OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
