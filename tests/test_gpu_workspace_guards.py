"""The Wilson-family entry points on workspaces of exactly their query's size (csrc/sc_workspace.h lays each out once, for the
query and for the entry point): sc_mvar_factor_f64, sc_granger_pairwise_f64 in both forms, sc_wilson_factor_f64,
sc_conditional_granger_f64 and sc_blockwise_granger_f64, at the smallest shapes that reach every branch of a layout
(tests/test_gpu_mvar_measures.py::test_nothing_is_stored_outside_the_buffers does the same for sc_mvar_measure_f64).

Each case runs the ordinary driver of spectral_connectivity_amd/_stage_d.py twice: on plain tensors, and on the memory of
tests/guarded_buffers.py, where the workspace and every output lie between two 4 KB bands of a pattern.  The bands survive, one
of the guarded arrays has exactly the query's byte count, and the outputs of the two runs are the same bits.  Then the query is
made to answer one byte less: the driver allocates and passes that, the call is refused, and neither the workspace nor an
output has been written."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chunked_calls                                                          # noqa: E402
import conditional_granger_ref as cref                                        # noqa: E402
from guarded_buffers import guarded_memory                                    # noqa: E402
from spectral_connectivity_amd import _lib                                    # noqa: E402

gpu = pytest.mark.gpu


def query(name, *args):
    nbytes = ctypes.c_size_t()
    _lib.check(getattr(_lib._handle(), name)(*args, ctypes.byref(nbytes)), name)
    return nbytes.value


def same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def check_entry(call, nbytes):
    """call(mem): the driver on the memory adapter ``mem``, returning (arrays ..., summary).  nbytes: the query's answer for
    the workspace of (each of) its library calls."""
    import torch
    from spectral_connectivity_amd import _stage_d, engine
    _lib.require_gpu()
    want = call(engine.TorchMemory(torch.device("cuda:0")))
    mem = guarded_memory()
    got = call(mem)
    torch.cuda.synchronize()
    assert nbytes in mem.sizes(), "no array of the query's size: the driver did not allocate the workspace as the query says"
    assert mem.intact(), "stored outside the workspace or an output"
    assert got[-1] == want[-1], "summaries differ"
    for k, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        assert same_bits(g, w), f"output {k} differs from the ordinary host path"
    short, size = guarded_memory(), _stage_d._size
    with chunked_calls.replaced(_stage_d, "_size", lambda fn, what, *args: size(fn, what, *args) - 1):
        with pytest.raises(_lib.HipEngineError, match="workspace too small"):
            call(short)
    torch.cuda.synchronize()
    assert nbytes - 1 in short.sizes()
    assert short.untouched() and short.intact(), "a refused call wrote"


def symmetric_spectra(P, N, C, seed):
    """[P][N][C][C] complex128 on the device: A A^H + I per bin, S(-f) = conj S(f) (real at f = 0 and at Nyquist)"""
    import torch
    rng = np.random.default_rng(seed)
    S = np.empty((P, N, C, C), dtype=np.complex128)
    for n in range(N // 2 + 1):
        A = rng.standard_normal((P, C, C)) / np.sqrt(C)
        if n not in (0, N - n):
            A = A + 1j * rng.standard_normal((P, C, C)) / np.sqrt(C)
        S[:, n] = A @ np.conj(np.swapaxes(A, -1, -2)) + np.eye(C)
        S[:, (N - n) % N] = np.conj(S[:, n])
    return torch.from_numpy(S).to("cuda:0")


@gpu
@pytest.mark.parametrize("C,N,P", [(5, 8, 2), (50, 8, 2), (130, 4, 1)])
def test_mvar_factor(C, N, P):
    """Up to 48 signals three series buffers, beyond them five, beyond 128 T doubles as the scratch of the blocked inverse."""
    from spectral_connectivity_amd import _stage_d
    S = symmetric_spectra(P, N, C, 100 + C)
    check_entry(lambda mem: _stage_d.mvar_factor(mem, P, N, C, spectra=S), query("sc_mvar_workspace_bytes", P, C, N))


def records(N, W=2, C=3):
    """(accum, n_obs, n_freq) of W windows of N samples of a real series, from the ordinary accumulate path"""
    import spectral_connectivity_amd as sc
    rng = np.random.default_rng(N)
    e = rng.standard_normal((N * W + 64, 4, C))
    x = np.zeros_like(e)
    for t in range(2, len(x)):
        x[t] = 0.5 * x[t - 1] - 0.3 * x[t - 2] + e[t]
        x[t, :, 1:] += 0.35 * x[t - 1, :, :-1]
    m = sc.Multitaper(x[64:], sampling_frequency=500.0, time_halfbandwidth_product=3, n_time_samples_per_window=N)
    accum, n_obs, n_freq = sc.Connectivity.from_multitaper(m)._csm_records("granger")
    assert n_freq == N // 2 + 1 and accum.shape[0] == W * n_freq
    return accum, n_obs, n_freq


@gpu
@pytest.mark.parametrize("N", [32, 256])
def test_granger_pairwise(N):
    """3 signals, all 3 pairs, 2 windows.  N = 32: the batched form (sc_wilson.hip); N = 256: the resident form
    (sc_wilson_pair.hip), which lays its own, smaller workspace into the same bytes."""
    from spectral_connectivity_amd import _stage_d
    accum, n_obs, n_freq = records(N)
    pairs = np.array([(0, 1), (0, 2), (1, 2)], dtype=np.int32)
    check_entry(lambda mem: _stage_d.granger_pairwise(mem, accum, 2, n_freq, N, 3, _lib.PLANE_CSM, n_obs, pairs),
                query("sc_granger_workspace_bytes", 2, 3, N))


@gpu
def test_wilson_factor():
    """3 problems of 32 bins through minimum_phase_decomposition, which takes its workspace from engine.TorchMemory."""
    import torch
    from spectral_connectivity_amd import engine
    from spectral_connectivity_amd.minimum_phase_decomposition import minimum_phase_decomposition
    S = symmetric_spectra(3, 32, 2, 7).cpu().numpy()

    def call(mem):
        with chunked_calls.replaced(engine, "TorchMemory", lambda device: mem):
            return torch.from_numpy(minimum_phase_decomposition(S)), None

    check_entry(call, query("sc_granger_workspace_bytes", 1, 3, 32))


@gpu
@pytest.mark.parametrize("C,N,n_dropped", [(5, 32, 2), (130, 4, 1)])
def test_conditional_granger(C, N, n_dropped):
    """5 signals, two dropped per call: the factorisation's workspace is the longer member of the tail.  130 signals, one
    dropped: 129 reduced signals, the blocked inverse's scratch in the tail behind K (four iterations: what is compared is
    bits, not convergence)."""
    import torch
    from spectral_connectivity_amd import _stage_d, engine
    if C == 5:
        A = np.zeros((2, C, C))
        A[0] = 0.3 * np.eye(C) + 0.25 * np.eye(C, k=-1)
        A[1, 0, 3] = 0.2
        S = torch.from_numpy(np.ascontiguousarray(cref.var_spectrum(A, np.eye(C), N)[None])).to("cuda:0")
    else:
        S = symmetric_spectra(1, N, C, 9)
    max_iterations = 60 if C == 5 else 4
    G = engine.mvar_factor(1, N, C, spectra=S, max_iterations=max_iterations)[0]
    nbytes = query("sc_conditional_granger_workspace_bytes", 1, C, N, n_dropped)

    def call(mem):
        with chunked_calls.replaced(_lib, "CONDITIONAL_WORK_BYTES", nbytes):
            return _stage_d.conditional_granger(mem, G, 1, N, C, spectra=S, max_iterations=max_iterations)

    check_entry(call, nbytes)


@gpu
@pytest.mark.parametrize("m,N,n_pairs", [(4, 32, 2), (66, 4, 1)])
def test_blockwise_granger(m, N, n_pairs):
    """Two pairs of 2 + 2 signals among 6; one pair of 33 + 33: beyond 64 signals bw_nullspace keeps Psi0 in the tail."""
    from spectral_connectivity_amd import _stage_d
    C = 6 if m == 4 else 66
    labels = [0, 0, 1, 1, 2, 2] if m == 4 else [0] * 33 + [1] * 33
    pairs = _lib.blockwise_pairs(labels, C, 512)[1][:n_pairs]
    batches, skipped = _lib.blockwise_batches(pairs, 1 << 20)
    assert not skipped and list(batches) == [m] and len(batches[m][1]) == n_pairs
    S = symmetric_spectra(2, N, C, 40 + m)
    check_entry(lambda mem: _stage_d.blockwise_granger(mem, 2, N, C, batches, len(set(labels)), spectra=S),
                query("sc_blockwise_granger_workspace_bytes", 2, m, N, n_pairs))
