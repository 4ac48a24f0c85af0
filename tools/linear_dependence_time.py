"""Device time of the total, instantaneous and lagged linear dependence (sc_linear_dependence_f64, all three outputs) for 7 windows
x 513 bins = 3591 records (1024-sample windows, float64 engine): 256 channels as 16 x 16, 8 x 32 and 4 x 64 groups and the pairwise
call at 128 channels, beside
  * the MIC + MIM call (sc_imaginary_interaction_f64) with the same groups on the same records, and
  * what a user has without it: torch.linalg.cholesky + log-diagonal of the same determinants on the same GPU -- per pair the
    joint block of S and of Re S (the leading-block identity gives ln det S_JJ - ln det S_aa from one factor, as in the kernel),
    per group its own block of both; the gather of the blocks is timed with it and also given alone.  Pairwise: the closed forms
    of the coherency, elementwise.

    python tools/linear_dependence_time.py [--out FILE]      # prints the table and writes it (default
                                                             # profiles/linear_dependence_time.txt)
Times are hipEvent intervals around the calls (records and matrices resident, best of 5)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spectral_connectivity_amd as sc                  # noqa: E402
from spectral_connectivity_amd import _lib, engine      # noqa: E402

WANT = ("total", "instantaneous", "lagged")
W, L, R = 7, 1024, 24                                   # 24 trials x 7 tapers = 168 observations (> 128 joint signals)
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn, reps=5):
    best, out = 1e30, None
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best, out


def records(C):
    """(CSM records [3591, ...] over 168 observations, n_obs, the same matrices [3591, C, C] complex128)."""
    rng = np.random.default_rng(9)
    x = rng.standard_normal((W * L, R, C)).astype(np.float32)
    x[1:, :, 1:] += 0.5 * x[:-1, :, :-1]
    m = sc.Multitaper(x, sampling_frequency=1000.0, time_halfbandwidth_product=4, n_time_samples_per_window=L,
                      n_time_samples_per_step=L)
    c = sc.Connectivity.from_multitaper(m, expectation_type="trials_tapers", dtype=np.complex128)
    sp = c._device()
    accum, n_obs = engine.accumulate(sp, "trials_tapers", _lib.PLANE_CSM, n_freq=c._n_freq)
    X = sp.coefficients()[:c._n_freq]                                                # (F, W, R, K, C)
    S = torch.empty((W, c._n_freq, C, C), dtype=torch.complex128, device=accum.device)
    for w in range(W):                                                               # (a window at a time: the product's workspace)
        Xw = X[:, w].reshape(c._n_freq, -1, C).to(torch.complex128)
        S[w] = torch.einsum("foi,foj->fij", Xw, Xw.conj()) / n_obs
    del X, sp, c
    return accum, n_obs, S.reshape(-1, C, C)


def log_tail(Lf, p):
    """2 sum_{k >= p} ln L_kk of a batch of factors."""
    return 2.0 * torch.log(torch.diagonal(Lf, dim1=-2, dim2=-1).real[..., p:]).sum(-1)


def gather(S, n_groups, size):
    """Joint blocks [n_bins, pairs, 2 size, 2 size] (a then b) and group blocks [n_bins, G, size, size] of contiguous groups."""
    ia, ib = torch.triu_indices(n_groups, n_groups, 1, device=S.device)
    ar = torch.arange(size, device=S.device)
    J = torch.cat([ia[:, None] * size + ar, ib[:, None] * size + ar], dim=1)        # [pairs, 2 size]
    Gi = torch.arange(n_groups, device=S.device)[:, None] * size + ar
    return S[:, J[:, :, None], J[:, None, :]], S[:, Gi[:, :, None], Gi[:, None, :]], ib


def torch_dependence(S, n_groups, size):
    joint, blocks, ib = gather(S, n_groups, size)
    tc, tr = log_tail(torch.linalg.cholesky(blocks), 0), log_tail(torch.linalg.cholesky(blocks.real), 0)
    total = tc[:, ib] - log_tail(torch.linalg.cholesky(joint), size)
    inst = tr[:, ib] - log_tail(torch.linalg.cholesky(joint.real), size)
    return total, inst, total - inst


def torch_pairwise(S):
    d = torch.sqrt(torch.diagonal(S, dim1=-2, dim2=-1).real)
    c = S / (d[:, :, None] * d[:, None, :])
    re2, im2 = c.real ** 2, c.imag ** 2
    return -torch.log1p(-(re2 + im2)), -torch.log1p(-re2), torch.log1p(im2 / (1.0 - (re2 + im2)))


def main():
    out_path = os.path.join(ROOT, "profiles", "linear_dependence_time.txt")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    say(f"{W} windows x {L // 2 + 1} bins = {W * (L // 2 + 1)} records, {R} trials x 7 tapers, float64 engine; ms, best of 5")
    say(f"{'shape':>22} {'sc_linear_dependence_f64':>25} {'MIC + MIM':>10} {'torch cholesky + logs':>22} {'(gather alone)':>15} "
        f"{'worst |difference|':>19}")
    accum, n_obs, S = records(256)
    for n_groups, size in ((16, 16), (8, 32), (4, 64)):
        members, sizes, _ = _lib.member_table([np.arange(g * size, (g + 1) * size) for g in range(n_groups)])
        t_dev, (res, n_fail) = timed(lambda: engine.linear_dependence(accum, 256, _lib.PLANE_CSM, n_obs, members, sizes, WANT))
        t_mic, _ = timed(lambda: engine.imaginary_interaction(accum, 256, _lib.PLANE_CSM, n_obs, members, sizes))
        t_ref, ref = timed(lambda: torch_dependence(S, n_groups, size))
        t_gather, _ = timed(lambda: gather(S, n_groups, size))
        ia, ib = torch.triu_indices(n_groups, n_groups, 1, device=S.device)
        diff = max((res[name][:, ia, ib] - r).abs().max().item() for name, r in zip(WANT, ref))
        say(f"{f'{n_groups} groups x {size}':>22} {t_dev:>25.3f} {t_mic:>10.3f} {t_ref:>22.3f} {t_gather:>15.3f} {diff:>19.2e}"
            f"   (n_fail {n_fail})")
        del res, ref
        torch.cuda.empty_cache()
    del accum, S
    torch.cuda.empty_cache()
    accum, n_obs, S = records(128)
    members, sizes, _ = _lib.member_table([np.array([c]) for c in range(128)])
    t_dev, (res, n_fail) = timed(lambda: engine.linear_dependence(accum, 128, _lib.PLANE_CSM, n_obs, members, sizes, WANT))
    t_lag, _ = timed(lambda: engine.linear_dependence(accum, 128, _lib.PLANE_CSM, n_obs, members, sizes, ("lagged",)))
    t_mic, _ = timed(lambda: engine.imaginary_interaction(accum, 128, _lib.PLANE_CSM, n_obs, members, sizes))
    t_ref, ref = timed(lambda: torch_pairwise(S))
    off = ~torch.eye(128, dtype=torch.bool, device=S.device)
    diff = max((res[name] - r)[:, off].abs().max().item() for name, r in zip(WANT, ref))
    say(f"{'pairwise, 128 signals':>22} {t_dev:>25.3f} {t_mic:>10.3f} {t_ref:>22.3f} {'-':>15} {diff:>19.2e}   (n_fail {n_fail}; "
        f"the lagged output alone, as lagged_coherence() asks: {t_lag:.3f} ms; torch: the closed forms, elementwise)")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
