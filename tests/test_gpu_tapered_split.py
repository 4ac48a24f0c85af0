"""Tapered split plans of stage B on the planes format (csrc/sc_fused_split.h, fu_part_range in csrc/sc_fused_common.h): a bin's
chunks cut into equal big parts and one short tail part, the big parts of all bins dispatched ahead of the tails.  The shapes are
small -- 33 bins of 36 ... 630 observations --, where the planner itself would never pick such a plan: SC_FUSED_SPLIT=n with
SC_FUSED_SPLIT_TAIL=t forces it.  And the parts-summing epilogue against the epilogue of the summed record.

Spectra as a 64-sample window gives them: F = 33 bins, one window, 3 tapers, `trials` trials -- 3 x trials observations per bin
in chunks of 32.  Reference and bound are those of tests/test_gpu_planes.py::test_stage_b_on_planes_three_term_sweep, which holds
them inline: float64 sums (tests/fp64_device_ref.py) of the same complex64-rounded coefficients, |err| <= 3e-6 |S_ij| + 2e-7
sqrt(P_i P_j) on every cross-spectrum of the upper triangle and 1e-5 relative on the sums of |Im s|."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import unpack_record_planes                                     # noqa: E402
from fp64_device_ref import sums_fp64                                         # noqa: E402
from spectral_connectivity_amd import _lib, engine                            # noqa: E402
from test_gpu_planes import PLANES, _planes_from_complex64                    # noqa: E402

F, W, K, OC = 33, 1, 3, 32
CSM_REL, CSM_PAIR, ABS_REL = 3e-6, 2e-7, 1e-5         # test_stage_b_on_planes_three_term_sweep's bound (see the module docstring)


@pytest.fixture(autouse=True)
def _planes_from_two_channels(monkeypatch):
    monkeypatch.setenv("SC_PLANES_MIN_CHANNELS", "2")


@functools.lru_cache(maxsize=None)
def _case(trials, C):
    """(planes-format spectra, complex128 coefficients [F, 1, n_obs, 1, C] of the same complex64-rounded numbers, float64 sums)."""
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100 * trials + C)
    coef = rng.standard_normal((F, W, trials, K, C)) + 1j * rng.standard_normal((F, W, trials, K, C))
    coef = coef + 0.4 * coef[..., :1]                                  # a shared component (before the scales: no cancelling pairs)
    coef = coef * (0.2 + rng.random(C)) * 10.0 ** rng.integers(-3, 4, C)
    X = torch.from_numpy(coef.astype(np.complex64)).to(dev)
    X64 = X.to(torch.complex128).reshape(F, W, trials * K, 1, C)       # observation o = trial * K + taper, as stage B counts them
    return _planes_from_complex64(X, C), X64, _sums(X64)


def _sums(X64):
    csm, ab = sums_fp64(X64)
    C = X64.shape[-1]
    return csm.cpu().numpy().reshape(F, C, C), ab.cpu().numpy().reshape(F, C, C)


def _worst(record, C, S, A):
    """Worst err / bound of a record [F, floats_per_bin] against the float64 sums: (cross-spectra, |Im s|)."""
    rec = unpack_record_planes(record.cpu().numpy(), C)                                    # [F, 3, C, C]
    Pw = np.real(np.einsum("fii->fi", S))
    pair = np.sqrt(Pw[:, :, None] * Pw[:, None, :])
    upper, strict = np.triu(np.ones((C, C), dtype=bool)), np.triu(np.ones((C, C), dtype=bool), 1)
    e_csm = (np.abs(rec[:, 0] + 1j * rec[:, 1] - S)[:, upper] / (CSM_REL * np.abs(S)[:, upper] + CSM_PAIR * pair[:, upper])).max()
    e_abs = (np.abs(rec[:, 2] - A)[:, strict] / A[:, strict]).max() / ABS_REL
    return e_csm, e_abs


# (trials, parts, tail chunks): 630 observations = 20 chunks as 18 + 2 (the big part crosses the 512-observation fold) and as
# 9 + 10 + 1; 615 observations: the tail part ends in a chunk of 7; 36 observations = 2 chunks (the second of 4 observations), whose
# only split is one chunk per part
CASES = [(210, 2, 2), (210, 3, 1), (205, 2, 2), (12, 2, 1)]


@pytest.mark.parametrize("C", [64, 96, 128])
@pytest.mark.parametrize("trials,n_parts,tail", CASES)
def test_tapered_parts_give_the_record(trials, n_parts, tail, C, debug_env):
    spp, X64, (S, A) = _case(trials, C)
    n_obs = trials * K
    n_chunks = (n_obs + OC - 1) // OC
    debug_env("SC_FUSED_SPLIT", n_parts)
    debug_env("SC_FUSED_SPLIT_TAIL", tail)
    accum, n = engine.accumulate(spp, "trials_tapers", PLANES)
    parts, _ = engine.accumulate(spp, "trials_tapers", PLANES, fold=False)
    assert n == n_obs and accum.dim() == 2 and parts.dim() == 3 and parts.shape[0] == n_parts
    which = [_lib.M_COHERENCE_MAGNITUDE, _lib.M_WPLI]
    from_parts = engine.measure_multi(parts, C, PLANES, n, which)
    from_record = engine.measure_multi(accum, C, PLANES, n, which)
    for a, b in zip(from_parts, from_record):
        assert torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), "the epilogue on the parts differs from the epilogue on the folded record"
    assert torch.equal(engine.fold_parts(parts), accum)
    e_csm, e_abs = _worst(accum, C, S, A)
    # the tail part alone holds the last `tail` chunks, the first part the first of the equally shared rest
    lo_tail = (n_chunks - tail) * OC
    e_tail = _worst(parts[n_parts - 1], C, *_sums(X64[:, :, lo_tail:]))
    hi_first = (n_chunks - tail) // (n_parts - 1) * OC
    e_first = _worst(parts[0], C, *_sums(X64[:, :, :hi_first]))
    print(f"\n  {trials} trials, {C} signals, {n_parts} parts, tail {tail}: err / bound (cross-spectra, |Im s|) record {e_csm:.3f} {e_abs:.3f}, "
          f"tail part {e_tail[0]:.3f} {e_tail[1]:.3f}, first part {e_first[0]:.3f} {e_first[1]:.3f}")
    assert e_csm <= 1.0 and e_abs <= 1.0, (e_csm, e_abs)
    assert max(e_tail) <= 1.0 and max(e_first) <= 1.0, (e_tail, e_first)


def test_equal_split_is_untouched_by_a_tail_of_zero(debug_env):
    """SC_FUSED_SPLIT alone keeps its meaning: n equal parts, whatever SC_FUSED_SPLIT_TAIL=0 or its absence says."""
    spp, _, _ = _case(210, 64)
    debug_env("SC_FUSED_SPLIT", 3)
    debug_env("SC_FUSED_SPLIT_TAIL", None)
    a, _ = engine.accumulate(spp, "trials_tapers", PLANES, fold=False)
    debug_env("SC_FUSED_SPLIT_TAIL", 0)
    b, _ = engine.accumulate(spp, "trials_tapers", PLANES, fold=False)
    assert a.shape[0] == 3 and torch.equal(a, b)


@pytest.mark.parametrize("C", [2, 17, 128])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 5])
def test_parts_epilogue_equals_the_epilogue_of_the_summed_record(n_parts, C):
    """measure_tile_multi_kernel on [n_parts] partial records against the same kernel on their sum in part order (float32, on the
    host side of the library: engine.fold_parts), bit for bit; 7 bins of synthetic records: normal cross terms, positive |Im s| sums,
    powers of 4 ... 5 per part on the diagonals (coherences spread over [0, 1])."""
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(17 * C + n_parts)
    n_bins, n_obs, NB = 7, 40 * n_parts, (C + 15) // 16
    n_tiles = NB * (NB + 1) // 2
    rec = torch.randn((n_parts, n_bins, 3, n_tiles, 16, 16), dtype=torch.float32, device=dev, generator=g)
    rec[:, :, 2] = rec[:, :, 2].abs() + 0.1
    d = torch.arange(16, device=dev)
    for bi in range(NB):
        t = bi * NB - bi * (bi - 1) // 2
        rec[:, :, 0, t, d, d] = 4.0 + torch.rand((n_parts, n_bins, 16), dtype=torch.float32, device=dev, generator=g)
    parts = rec.reshape(n_parts, n_bins, 3 * n_tiles * 256).contiguous()
    which = [_lib.M_COHERENCE_MAGNITUDE, _lib.M_WPLI]
    got = engine.measure_multi(parts, C, PLANES, n_obs, which)
    want = engine.measure_multi(engine.fold_parts(parts).clone(), C, PLANES, n_obs, which)
    for a, b, name in zip(got, want, ("coherence", "wPLI")):
        assert a.shape == (n_bins, C, C)
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num()), name
        assert bool(torch.isfinite(a[:, 0, C - 1]).all()) and float(a.nan_to_num().abs().max()) > 0
