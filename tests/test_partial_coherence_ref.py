"""CPU-only checks of the NumPy reference of partial and multiple coherence (tests/partial_coherence_ref.py) that the device
tests compare against: its two forms -- the inverse of the cross-spectral matrix, and the coherency of the residuals after
regressing each pair on all other channels -- share no step and agree; two signals give the ordinary coherency; a positive
diagonal scaling changes nothing; a common driver leaves no partial coherence."""
import numpy as np
import pytest

import partial_coherence_ref as pref
from test_gpu_imaginary_interaction import var_spectrum


@pytest.mark.parametrize("C", [2, 3, 7, 17])
def test_the_two_forms_agree(C):
    S = var_spectrum(C, C)
    cond = np.linalg.cond(S)
    assert 1.0 < cond.min() and cond.max() < 100.0            # (well conditioned: the 1e-12 below is rounding, not luck)
    gi, ri = pref.inverse(S)
    gr, rr = pref.residual(S)
    assert gi.shape == gr.shape == S.shape and ri.shape == rr.shape == S.shape[:-1]
    off = ~np.eye(C, dtype=bool)
    assert np.isnan(gi[:, ~off]).all() and np.isnan(gr[:, ~off]).all()
    assert np.abs(gi[:, off] - gr[:, off]).max() <= 1e-12
    assert np.abs(ri - rr).max() <= 1e-12
    # Hermitian (to the rounding of an unsymmetric LU inverse: the bound of the two forms), inside the unit disc, not trivially zero
    assert np.abs(gi[:, off] - np.conj(np.swapaxes(gi, -1, -2))[:, off]).max() <= 1e-12
    assert np.abs(gi[:, off]).max() <= 1.0 and np.abs(gi[:, off]).max() > 0.05
    assert ri.min() >= 0.0 and ri.max() < 1.0 and ri.max() > 0.1


def test_two_signals_give_the_ordinary_coherency():
    S = var_spectrum(2, 4)
    for form in (pref.inverse, pref.residual):
        gamma, multiple = form(S)
        coh = pref.coherency(S)
        assert np.abs(gamma[:, 0, 1] - coh[:, 0, 1]).max() <= 1e-14
        assert np.abs(gamma[:, 1, 0] - coh[:, 1, 0]).max() <= 1e-14
        # one other channel explains |coherency|^2 of the power
        assert np.abs(multiple - np.abs(coh[:, 0, 1])[:, None]).max() <= 1e-14
    assert np.abs(coh[1:-1, 0, 1].imag).max() > 1e-3           # (the sign of the phase is pinned, not only the magnitude)


def test_invariant_under_diagonal_scaling():
    C = 7
    S = var_spectrum(C, 11)
    d = 10.0 ** (3.0 * np.arange(C) / C - 1.5)
    scaled = d[None, :, None] * S * d[None, None, :]
    for form in (pref.inverse, pref.residual):
        a, ra = form(S)
        b, rb = form(scaled)
        off = ~np.eye(C, dtype=bool)
        assert np.abs(a[:, off] - b[:, off]).max() <= 1e-12
        assert np.abs(ra - rb).max() <= 1e-12


def test_common_driver_leaves_no_partial_coherence():
    S, sigma, (s1, s2) = pref.common_driver_spectrum()
    ordinary = np.abs(pref.coherency(S)[:, 0, 1])
    assert np.abs(ordinary - sigma / np.sqrt((sigma + s1) * (sigma + s2))).max() <= 1e-14
    assert ordinary.min() > 0.2
    q = 1.0 / s1 + 1.0 / s2
    for form in (pref.inverse, pref.residual):
        gamma, multiple = form(S)
        assert np.abs(gamma[:, 0, 1]).max() <= 1e-14
        assert np.abs(multiple[:, 2] - np.sqrt(sigma * q / (1.0 + sigma * q))).max() <= 1e-13
        # what is left between each noisy copy and the driver is the whole of their coupling
        assert np.abs(gamma[:, 0, 2]).min() > 0.2
