"""Connectivity measures: host-side mirror of the reference's ``Connectivity`` API.

Same constructor, properties, method names, output shapes (NumPy float64 / complex128,
non-negative frequencies only) and error behaviour as
``spectral_connectivity.connectivity.Connectivity`` (reference connectivity.py:163-1650) for
the hot-path measures.  All arithmetic runs on an MI355X through ``libsc_hip.so``:

    expectation of the cross-spectral matrix and the per-observation planes |Im s|, (Im s)^2, sign Im s, s/|s|
        float32 engine (dtype=complex64): one pass on the bf16 matrix pipe, bf16x3 split (sc_fused.hip), an f32 VALU kernel
                       for few channels, the f32-MFMA / per-plane VALU kernels for strided spectra (sc_csm.hip, sc_nonlinear.hip)
        float64 engine (dtype=complex128, the default): fp64 matrix cores + fp64 VALU, double records (sc_f64.hip)
    measure algebra, eps clamps, NaN diagonals  -> fp64 epilogue, several measures per launch (sc_measure.hip)
    pairwise Granger / full Wilson + MVAR measures / canonical / global coherence / MIC, MIM -> sc_wilson.hip, sc_wilson_fft.hip,
        sc_mvar.hip, sc_canonical.hip, sc_global.hip (fp64)

There is no NumPy fallback: without the HIP extension / a GPU every measure raises.
"""
import warnings
from collections import namedtuple
from logging import getLogger

import numpy as np

from . import _lib
from ._lib import EXPECTATION_AXES

# scale of the Tikhonov terms in the MVAR quantities (reference connectivity.py: same name and value; applied on the
# device in sc_mvar.hip / sc_wilson.hip)
TIKHONOV_REGULARIZATION_FACTOR = 1e-12

logger = getLogger(__name__)

# kept for API parity with reference connectivity.py:67-75 (keys are what matters)
EXPECTATION = dict.fromkeys(EXPECTATION_AXES)

# what maximized_imaginary_coherence_vectors returns
InteractionVectors = namedtuple("InteractionVectors", ("mic", "filters", "patterns", "labels", "members"))
CanonicalVectors = namedtuple("CanonicalVectors", ("coherence", "coherences", "filters", "patterns", "labels", "members"))
LinearDependence = namedtuple("LinearDependence", ("total", "instantaneous", "lagged", "labels"))
SeedConnectivity = namedtuple("SeedConnectivity", ("values", "seeds", "targets"))
SeedJackknife = namedtuple("SeedJackknife", ("results", "seeds", "targets"))


class _PendingSpectra:
    """A float32-engine transform that has not run yet (Connectivity.from_multitaper): sizes only."""

    def __init__(self, multitaper, precision):
        self.multitaper, self.precision = multitaper, precision
        shape = multitaper.time_series.shape
        self.shape5 = (int(multitaper.n_time_windows), int(shape[1]), int(multitaper.n_tapers),
                       int(multitaper.n_fft_samples), int(shape[2]))


class Connectivity:
    """Frequency-domain connectivity measures computed on an MI355X.

    Parameters mirror reference connectivity.py:277-285.  ``fourier_coefficients`` is either
    a 5-D complex array (n_time_windows, n_trials, n_tapers, n_fft_samples, n_signals) --
    uploaded once -- or, through :meth:`from_multitaper`, the HBM-resident spectra of a
    :class:`~spectral_connectivity_amd.transforms.Multitaper` (no host round trip).

    ``blocks`` is accepted for compatibility and ignored: the engine never materialises the
    per-observation cross-spectra the reference blocks over.

    ``dtype`` selects the device arithmetic, as it selects the arithmetic of the reference's cross-spectral products
    (connectivity.py:277-285, :1799-1822): ``numpy.complex128`` (the default, like the reference) runs the float64
    engine -- float64 transform, cross-spectra on the fp64 matrix cores, float64 measures: results equal to the
    reference's to ~1e-12 --, ``numpy.complex64`` the float32 engine of the headline path (fused f32 transform, bf16x3
    / f32 matrix cores, fp64 epilogue: ~1e-6 on power, ~1e-7 of the array maximum on cross-spectral measures, 2-3x
    faster).  ``options.precision`` can force either engine for the whole process.
    """

    def __init__(self, fourier_coefficients, expectation_type="trials_tapers", frequencies=None,
                 time=None, blocks=None, dtype=np.complex128):
        from . import options
        self._precision = options.engine_precision(dtype)
        self._spectra = None
        self._pending = None
        self._deferred_source = None      # (Multitaper, precision) whose transform left checks pending: _settle
        self._host_coefficients = None
        self._multitaper = None
        if getattr(fourier_coefficients, "is_device_spectra", False):
            self._spectra = fourier_coefficients
        elif isinstance(fourier_coefficients, _PendingSpectra):
            self._pending = fourier_coefficients
        else:
            fourier_coefficients = np.asarray(fourier_coefficients)
            if fourier_coefficients.ndim != 5:
                raise ValueError(
                    f"fourier_coefficients must be 5-dimensional, got {fourier_coefficients.ndim}D array.\n"
                    "Expected shape: (n_time_windows, n_trials, n_tapers, n_fft_samples, n_signals)\n"
                    f"Got shape: {fourier_coefficients.shape}\n\n"
                    "If you have time series data, use the Multitaper class to transform it:\n"
                    "  from spectral_connectivity_amd import Multitaper\n"
                    "  m = Multitaper(time_series, sampling_frequency=your_fs, ...)\n"
                    "  fourier_coefficients = m.fft()")
            self._host_coefficients = fourier_coefficients
        if expectation_type not in EXPECTATION_AXES:
            words = set(expectation_type.split("_"))
            suggestion = None
            if words.issubset({"time", "trials", "tapers"}):
                for key in EXPECTATION_AXES:
                    if set(key.split("_")) == words:
                        suggestion = key
                        break
            msg = (f"Invalid expectation_type '{expectation_type}' is not supported.\n"
                   "This parameter controls which dimensions to average over when computing "
                   "the cross-spectral matrix.\n")
            if suggestion:
                msg += f"\nDid you mean '{suggestion}'? (The words must be in a specific order)\n"
            msg += "\nValid options are:\n" + "".join(f"  - '{k}'\n" for k in sorted(EXPECTATION_AXES))
            msg += "\nMost common: 'trials_tapers' (average over both trials and tapers)"
            raise ValueError(msg)
        if self._host_coefficients is not None and not np.all(np.isfinite(self._host_coefficients)):
            warnings.warn(
                "fourier_coefficients contains NaN or Inf values. This may indicate:\n"
                "  - NaN/Inf in your input time series data\n"
                "  - Issues with windowing parameters (e.g., window too short)\n"
                "  - Numerical instability in preprocessing", UserWarning, stacklevel=2)
        self.expectation_type = expectation_type
        self._frequencies = frequencies
        self._blocks = blocks
        self._dtype = dtype
        self.time = None if time is None else np.asarray(time)
        self._accum_cache = {}

    @classmethod
    def from_multitaper(cls, multitaper_instance, expectation_type="trials_tapers", blocks=None,
                        dtype=np.complex128):
        """Reference connectivity.py:366-400, but the coefficients never leave the device."""
        from . import options
        precision = options.engine_precision(dtype)
        if precision == "float32" and not np.iscomplexobj(multitaper_instance.time_series):
            # float32 engine: the transform runs when the first measure asks for its accumulators -- which families they
            # are decides the device format of the spectra (CSM / |Im s|: f16 pieces for sc_fused2.hip, engine.multitaper_spectra)
            multitaper_instance.check_device_path()
            obj = cls(_PendingSpectra(multitaper_instance, precision), expectation_type=expectation_type,
                      time=multitaper_instance.time, frequencies=multitaper_instance.frequencies, blocks=blocks, dtype=dtype)
        else:
            obj = cls(multitaper_instance.device_spectra(precision=precision),
                      expectation_type=expectation_type, time=multitaper_instance.time,
                      frequencies=multitaper_instance.frequencies, blocks=blocks, dtype=dtype)
        obj._multitaper = multitaper_instance
        return obj

    # ---- bookkeeping ---------------------------------------------------------------------
    @property
    def fourier_coefficients(self):
        if self._host_coefficients is None:
            self._host_coefficients = self._multitaper.fft()
        return self._host_coefficients

    @property
    def _shape5(self):
        if self._host_coefficients is not None:
            return self._host_coefficients.shape
        if self._spectra is None and self._pending is not None:
            return self._pending.shape5
        s = self._spectra
        return (s.W, s.R, s.K, s.n_fft, s.C)

    @property
    def frequencies(self):
        """Non-negative frequencies (reference connectivity.py:402-424)."""
        if self._frequencies is None:
            return None
        f = np.asarray(self._frequencies)
        out = np.array(f[: len(f) // 2 + 1], dtype=float)
        if len(out) and out[-1] < 0:
            out[-1] = abs(out[-1])
        return out

    @property
    def all_frequencies(self):
        return None if self._frequencies is None else np.asarray(self._frequencies)

    @property
    def n_observations(self):
        """Reference connectivity.py:594-610."""
        return int(np.prod([self._shape5[a] for a in EXPECTATION_AXES[self.expectation_type]]))

    # ---- device plumbing -----------------------------------------------------------------
    def _planes_request_ok(self, planes):
        """Would the planes-format stage B (sc_fused2.hip) take ``planes`` with this object's expectation type and shape?  Asked
        BEFORE a pending transform picks the device format of the spectra: its observations must form one run of rows (every
        expectation type but "time_tapers" with several trials)."""
        from . import _stage_abc
        W, R, K, N, C = (int(v) for v in self._shape5)
        return _stage_abc.planes_request_ok(W, R, K, N, _lib.padded_channels(C, _lib.PLANES_FORMAT_MAX_CHANNELS), self.expectation_type,
                                            planes)

    def _settle(self):
        """Settle what the transform left pending (Multitaper.settle_device_checks: the deferred NaN / infinity warning, the planes
        format's quality check) -- called where a result is downloaded anyway.  False: the spectra were replaced (complex64 instead
        of the planes format) and everything computed from the old ones is dropped; the caller computes again."""
        src = self._deferred_source
        if src is None:
            return True
        self._deferred_source = None
        m, precision = src
        if m.settle_device_checks(precision):
            return True
        self._spectra = m.device_spectra(precision=precision)
        self._accum_cache.clear()
        return False

    def _device(self, planes_hint=None, defer_checks=False):
        """The device spectra; ``planes_hint``: the accumulator families about to be requested.  A pending transform writes the
        planes format when the SHAPE qualifies for it and the hint is one of the families its kernels serve -- whichever
        (_lib.planes_format_applies) -- and this object's expectation type can run on it.  ``defer_checks``: the caller downloads a
        result next and calls _settle() there (and computes again if that says so); every other caller gets settled spectra."""
        if self._spectra is None and self._pending is not None:
            if planes_hint is not None and not (planes_hint in _lib.PLANES_FORMAT_FAMILIES and self._planes_request_ok(planes_hint)):
                planes_hint = None
            m, precision = self._pending.multitaper, self._pending.precision
            self._spectra = m.device_spectra(precision=precision, planes_hint=planes_hint, defer_checks=True)
            self._deferred_source = (m, precision)
            self._pending = None
        if not defer_checks and self._deferred_source is not None:
            self._settle()
        if self._spectra is None:
            from . import engine
            _lib.require_gpu()
            self._spectra = engine.upload_coefficients(self._host_coefficients, f64=self._precision == "float64")
        return self._spectra

    @property
    def _n_freq(self):
        return self._shape5[3] // 2 + 1

    def _accumulators(self, planes, defer_checks=False):
        """Accumulator record containing at least ``planes`` (cached)."""
        from . import engine
        for have, rec in self._accum_cache.items():
            if isinstance(have, int) and have & planes == planes:
                return have, rec
        sp = self._device(planes_hint=planes, defer_checks=defer_checks)
        have = None
        single = self._reduce_over_ranks.__func__ is Connectivity._reduce_over_ranks
        if sp.f64 and single:
            # float64 engine, single process: families a cached record already holds are copied, not recomputed
            best = max((h for h in self._accum_cache if isinstance(h, int) and h & planes), key=lambda h: bin(h & planes).count("1"),
                       default=None)
            if best is not None:
                planes |= best                     # the new record supersedes the old one
                have = (best, self._accum_cache[best][0])
        from . import options
        if (sp.P is not None and planes == _lib.PLANE_CSM and options.anticipate_phase_lag
                and self._planes_request_ok(_lib.PLANE_CSM | _lib.PLANE_ABS_IM)):
            # spectra held as f16 pieces: the launch that sums the cross-spectra also sums |Im s| (options.anticipate_phase_lag) --
            # coherence followed by wPLI, the BASELINE pair, is then ONE pass over the spectra whichever comes first
            planes = _lib.PLANE_CSM | _lib.PLANE_ABS_IM
        # single process, float32 engine on the planes format: the split-bin partial records stay unfolded (a 3-D tensor) and
        # the epilogue sums them while it reads -- the path bench.py times
        accum, n_obs = engine.accumulate(self._guard_spectra(sp, planes), self.expectation_type, planes, n_freq=self._n_freq, have=have,
                                         fold=not single, guard=False)
        accum = self._reduce_over_ranks(accum)
        if have is not None:
            del self._accum_cache[have[0]]
        for old in [h for h in self._accum_cache if isinstance(h, int) and h & planes == h]:
            del self._accum_cache[old]              # a record the new one covers: its memory can go
        self._accum_cache[planes] = (accum, n_obs)
        return planes, (accum, n_obs)

    def _csm_records(self, tag, expectation_type=None, two_sided=True):
        """CSM records for the consumers that read every bin (Granger, MVAR, global / canonical coherence), cached and
        summed over the trial shards: (records, n_observations of this process, bins per group).  ``two_sided``:
        uploaded coefficients are accumulated on all N bins (real-input spectra hold 0..N/2, mirrored on the device)."""
        from . import engine
        sp = self._device()
        N = self._shape5[3]
        n_freq = (sp.F if sp.real_input else N) if two_sided else self._n_freq
        key = (tag, n_freq)
        if key not in self._accum_cache:
            accum, n_obs = engine.accumulate(sp, expectation_type or self.expectation_type, _lib.PLANE_CSM, n_freq=n_freq)
            self._accum_cache[key] = (self._reduce_over_ranks(accum), n_obs)
        accum, n_obs = self._accum_cache[key]
        return accum, n_obs, n_freq

    def _guard_spectra(self, sp, planes):
        """The spectra this request is accumulated from: a complex128 copy when (Im s)^2 or s / |s| would leave the float32 range
        (engine.guarded_spectra); parallel.ShardedConnectivity takes the decision once for its group."""
        from . import engine
        return engine.guarded_spectra(sp, planes)

    def _reduce_over_ranks(self, accum):
        """Sum of the records over the processes that hold the trials: nothing to add here; parallel.ShardedConnectivity
        (one process per GPU, trials sharded) all-reduces."""
        return accum

    def _memory(self, like):
        """The memory adapter of the stage-D drivers (_stage_d.py) on the host in use -- here the PyTorch host's, for the device
        of the tensor ``like``; its ``download`` brings a result to NumPy."""
        from . import engine
        return engine.TorchMemory(like.device)

    def _wilson_done(self, mem, noun, summary, n_iter, status):
        """The warnings of a batch of Wilson factorisations (``noun``: what one problem is) and ``_last_wilson``."""
        iters, not_conv, fallback = (int(v) for v in summary)
        n_iter, status = mem.download(n_iter), mem.download(status)
        if fallback:
            # reference minimum_phase_decomposition.py:78-93 (there the start is a random draw around the identity)
            logger.warning("Computing the initial conditions using the Cholesky failed. "
                           f"Using the identity as initial condition ({fallback} {noun}).")
        if not_conv:
            logger.warning(f"Maximum iterations reached. {status.size - not_conv} of {status.size} converged")
        self._last_wilson = dict(iterations=iters, not_converged=not_conv, cholesky_fallbacks=fallback, n_iter=n_iter, status=status)

    def _kept_shape(self):
        W, R, K = self._shape5[:3]
        axes = EXPECTATION_AXES[self.expectation_type]
        return tuple(n for i, n in enumerate((W, R, K)) if i not in axes)

    def _measure(self, which):
        from . import engine
        C = self._shape5[4]
        for _ in range(2):
            # (a fresh transform's two small read-backs are settled with this download, not before stage B: _settle; in the rare
            #  case the planes format is withdrawn there, the measure is computed once more from the complex64 spectra)
            have, (accum, n_obs) = self._accumulators(_lib.MEASURE_PLANES[which], defer_checks=True)
            # the epilogue writes the dtype the reference returns (_wide_output) itself: no widening pass on the way out
            host = engine.to_host(engine.measure(accum, C, have, self._n_observations_total(n_obs), which,
                                                 wide=self._wide_output(which)))
            if self._settle():
                break
        tail = (C,) if which == _lib.M_POWER else (C, C)
        return host.reshape(self._kept_shape() + (self._n_freq,) + tail)

    def _n_observations_total(self, local_n_obs):
        return local_n_obs

    # the measures whose arithmetic the reference runs in `dtype` from the first product on (the per-observation
    # cross-spectra of _complex_inner_product(dtype=...), connectivity.py:1799-1822, then fcn and the expectation)
    _DTYPE_MEASURES = frozenset((_lib.M_PLV, _lib.M_PLV_COMPLEX, _lib.M_PLI, _lib.M_WPLI, _lib.M_DEBIASED_PLI2,
                                 _lib.M_DEBIASED_WPLI2, _lib.M_PPC))

    def _wide_output(self, which):
        """True: float64 / complex128 results, False: float32 / complex64 -- what the reference returns for this
        measure: the phase-lag / phase-locking family comes out in the real type of ``dtype`` (float32 for
        ``dtype=complex64``); power and the coherency family divide by the power, which is computed from the
        coefficients themselves, so they come out in the coefficients' precision (complex128 from ``Multitaper.fft``,
        whatever ``dtype`` says; float32 only for uploaded complex64 coefficients)."""
        if which in self._DTYPE_MEASURES:
            return np.dtype(self._dtype) != np.complex64
        if self._multitaper is None and self._host_coefficients is not None:
            return self._host_coefficients.dtype != np.complex64
        return True

    # accumulator families behind the expectation-type measures of the public interface
    _METHOD_PLANES = {
        "power": _lib.PLANE_CSM, "coherency": _lib.PLANE_CSM, "coherence_phase": _lib.PLANE_CSM,
        "coherence_magnitude": _lib.PLANE_CSM, "imaginary_coherence": _lib.PLANE_CSM,
        "phase_locking_value": _lib.PLANE_UNIT, "pairwise_phase_consistency": _lib.PLANE_UNIT,
        "phase_lag_index": _lib.PLANE_SIGN_IM, "debiased_squared_phase_lag_index": _lib.PLANE_SIGN_IM,
        "weighted_phase_lag_index": _lib.PLANE_CSM | _lib.PLANE_ABS_IM,
        "debiased_squared_weighted_phase_lag_index": _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ,
        "phase_slope_index": _lib.PLANE_CSM, "group_delay": _lib.PLANE_CSM, "delay": _lib.PLANE_CSM,
    }

    def _prepare(self, methods):
        """The accumulator families the named measures need, each accumulated ONCE up front instead of a record per measure that
        re-accumulates what it shares with the others.  float32 engine: one record per kernel family -- the cross-spectral one
        (CSM, + |Im s|, + (Im s)^2: one launch, or one + a plane pass), sign(Im s), the unit phasors -- because each family is its
        own pass over the spectra anyway and the planes-format kernels take exactly these sets (a combined CSM + sign record would
        push the whole object back to complex64 spectra); float64 engine: one record (its kernels fill any subset, and a later
        request copies what a record already holds)."""
        planes = 0
        for name in methods:
            planes |= self._METHOD_PLANES.get(name, 0)
        if not planes or bin(planes).count("1") < 2:
            return
        if self._precision == "float64":
            self._accumulators(planes)
            return
        cross = _lib.PLANE_CSM | _lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ
        for family in (planes & cross, planes & _lib.PLANE_SIGN_IM, planes & _lib.PLANE_UNIT):
            if family & (_lib.PLANE_ABS_IM | _lib.PLANE_IM_SQ):
                family |= _lib.PLANE_CSM                       # (the |Im s| / (Im s)^2 planes ride on the cross-spectral launch)
            if family & _lib.PLANE_IM_SQ:
                family |= _lib.PLANE_ABS_IM
            if family and bin(family).count("1") > 1:
                self._accumulators(family)

    # ---- measures (reference connectivity.py:612-1159) -----------------------------------
    def power(self):
        """Power spectral density, non-negative frequencies: (..., n_freq, n_signals)."""
        return self._measure(_lib.M_POWER)

    def _expectation_cross_spectral_matrix(self):
        """E[X_i conj X_j] on the non-negative bins (reference connectivity.py:463-526)."""
        return self._measure(_lib.M_CSM)

    def coherency(self):
        return self._measure(_lib.M_COHERENCY)

    def coherence_phase(self):
        return self._measure(_lib.M_COHERENCE_PHASE)

    def coherence_magnitude(self):
        return self._measure(_lib.M_COHERENCE_MAGNITUDE)

    def imaginary_coherence(self):
        return self._measure(_lib.M_IMAGINARY_COHERENCE)

    def _phase_locking_value(self):
        return self._measure(_lib.M_PLV_COMPLEX)

    def phase_locking_value(self):
        return self._measure(_lib.M_PLV)

    def phase_lag_index(self):
        return self._measure(_lib.M_PLI)

    def weighted_phase_lag_index(self):
        return self._measure(_lib.M_WPLI)

    def debiased_squared_phase_lag_index(self):
        return self._measure(_lib.M_DEBIASED_PLI2)

    def debiased_squared_weighted_phase_lag_index(self):
        return self._measure(_lib.M_DEBIASED_WPLI2)

    def pairwise_phase_consistency(self):
        return self._measure(_lib.M_PPC)

    # ---- pairwise spectral Granger (reference connectivity.py:1161-1213) -----------------
    def _granger(self, pairs):
        N, C = self._shape5[3], self._shape5[4]
        out = self._granger_device(pairs)
        return self._memory(out).download(out).reshape(self._kept_shape() + (N // 2 + 1, C, C))

    def _granger_device(self, pairs):
        """Device array [n_groups, N/2+1, C, C] float64: the listed pairs filled in, NaN elsewhere."""
        from . import _stage_d
        N, C = self._shape5[3], self._shape5[4]
        accum, n_obs, n_freq = self._csm_records("granger")
        mem = self._memory(accum)
        out, n_iter, status, summary = _stage_d.granger_pairwise(mem, accum, accum.shape[0] // n_freq, n_freq, N, C, _lib.PLANE_CSM,
                                                                 self._n_observations_total(n_obs), pairs)
        self._wilson_done(mem, "problems", summary, n_iter, status)
        return out

    def pairwise_spectral_granger_prediction(self):
        """Power at node i explained by node j, out[..., i, j] = j -> i (diagonal NaN)."""
        C = self._shape5[4]
        pairs = np.array([(i, j) for i in range(C) for j in range(i + 1, C)], dtype=np.int32)
        if pairs.size == 0:
            return np.full(self._kept_shape() + (self._n_freq, C, C), np.nan)
        return self._granger(pairs)

    def subset_pairwise_spectral_granger_prediction(self, pairs):
        """Granger prediction for the listed (i, j) channel pairs only; every other entry is NaN
        (reference connectivity.py:1193-1213).  Indices follow NumPy rules: negative indices count from the end,
        anything outside [-n_signals, n_signals) raises IndexError."""
        C = self._shape5[4]
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            return np.full(self._kept_shape() + (self._n_freq, C, C), np.nan)
        if pairs.ndim != 2 or pairs.shape[1] != 2:
            raise ValueError(f"pairs must be a sequence of (i, j) index pairs, got shape {pairs.shape}")
        if not np.issubdtype(pairs.dtype, np.integer):
            if not np.all(pairs == np.floor(pairs)):
                raise IndexError("pair indices must be integers")
            pairs = pairs.astype(np.int64)
        bad = (pairs < -C) | (pairs >= C)
        if bad.any():
            raise IndexError(f"index {int(pairs[bad][0])} is out of bounds for axis with size {C}")
        pairs = np.where(pairs < 0, pairs + C, pairs).astype(np.int32)
        # a channel paired with itself is a singular 2 x 2 problem; its only entries lie on the (NaN) diagonal
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        if pairs.size == 0:
            return np.full(self._kept_shape() + (self._n_freq, C, C), np.nan)
        return self._granger(pairs)

    # ---- full Wilson factor and the directed MVAR measures (reference connectivity.py:567-589,
    # :1237-1426): one batched C x C factorisation on the device, cached, then one small kernel
    # per measure ------------------------------------------------------------------------------
    def _check_mvar_signals(self):
        C = self._shape5[4]
        if C > _lib.load().sc_mvar_max_signals():
            raise ValueError(f"the full Wilson factorisation supports n_signals <= "
                             f"{_lib.load().sc_mvar_max_signals()} (got {C}); use the pairwise measures")

    def _mvar_factor_device(self):
        from . import _stage_d
        if getattr(self, "_mvar_G", None) is not None:
            return self._mvar_G
        N, C = self._shape5[3], self._shape5[4]
        self._check_mvar_signals()
        accum, n_obs, n_freq = self._csm_records("granger")
        mem = self._memory(accum)
        G, n_iter, status, summary = _stage_d.mvar_factor(mem, accum.shape[0] // n_freq, N, C, accum=accum, n_freq_accum=n_freq,
                                                          planes=_lib.PLANE_CSM, n_obs=self._n_observations_total(n_obs))
        self._wilson_done(mem, "windows", summary, n_iter, status)
        self._mvar_G = G
        return G

    def _mvar(self, which, n_freq_axis=True):
        from . import _stage_d
        G = self._mvar_factor_device()
        mem = self._memory(G)
        out = mem.download(_stage_d.mvar_measure(mem, G, which))
        return out.reshape(self._kept_shape() + out.shape[1:])

    @property
    def _minimum_phase_factor(self):
        G = self._mvar_factor_device()
        G = self._memory(G).download(G)
        return G.reshape(self._kept_shape() + G.shape[1:])

    @property
    def _transfer_function(self):
        return self._mvar(_lib.MVAR_TRANSFER)

    @property
    def _noise_covariance(self):
        return self._mvar(_lib.MVAR_NOISE_COVARIANCE, n_freq_axis=False)

    @property
    def _MVAR_Fourier_coefficients(self):
        return self._mvar(_lib.MVAR_COEFFICIENTS)

    def directed_transfer_function(self):
        """|H_ij|^2 normalised by the total inflow into node i; out[..., i, j] = j -> i, range [0, 1]."""
        return self._mvar(_lib.MVAR_DTF)

    def directed_coherence(self):
        """Transfer-function coupling scaled by the noise variance, normalised by the inflow."""
        return self._mvar(_lib.MVAR_DC)

    def partial_directed_coherence(self, keep_cupy=False):
        """|A_ij|^2 of the MVAR Fourier coefficients normalised by the total outflow of node j."""
        return self._mvar(_lib.MVAR_PDC)

    def generalized_partial_directed_coherence(self):
        """Partial directed coherence with every row scaled by its noise variance."""
        return self._mvar(_lib.MVAR_GPDC)

    def direct_directed_transfer_function(self):
        """Full-frequency directed transfer function times sqrt(partial directed coherence)."""
        return self._mvar(_lib.MVAR_DDTF)

    # ---- band statistics of the coherency (reference connectivity.py:1428-1650): host-side post-processing
    # of the device coherency, see _postprocess.py ----------------------------------------------------
    def phase_slope_index(self, frequencies_of_interest=None, frequency_resolution=None):
        """Weighted average of the coherency phase slope projected on the imaginary axis (Nolte et al. 2008);
        out[..., i, j] > 0 when i leads j.  Shape (..., n_signals, n_signals)."""
        from . import _postprocess as pp
        return pp.phase_slope_index(self.coherency(), self.frequencies, frequencies_of_interest, frequency_resolution)

    def group_delay(self, frequencies_of_interest=None, frequency_resolution=None, significance_threshold=0.05):
        """Average time delay of a broadband signal between every pair: (delay, slope, r_value) from the linear
        regression of the unwrapped coherence phase on frequency over the significant bins of the band."""
        from . import _postprocess as pp
        return pp.group_delay(self.coherency(), self.frequencies, self.n_observations, frequencies_of_interest,
                              frequency_resolution, significance_threshold)

    def delay(self, frequencies_of_interest=None, frequency_resolution=None, significance_threshold=0.05, n_range=3):
        """Range of possible delays (2 pi ambiguity of the coherence phase) per band frequency and pair."""
        from . import _postprocess as pp
        return pp.delay(self.coherency(), self.frequencies, self.n_observations, frequencies_of_interest,
                        frequency_resolution, significance_threshold, n_range)

    # ---- global coherence (reference connectivity.py:822-895) ------------------------------
    def global_coherence(self, max_rank=1):
        """Leading squared singular values (/ n_estimates) and left singular vectors of the signals x
        (trials * tapers) coefficient matrix, per time window and (two-sided) frequency bin.

        Returns (values (n_time_windows, n_fft_samples, max_rank), vectors (n_time_windows,
        n_fft_samples, n_signals, max_rank)).  Computed as the leading eigenpairs of the cross-spectral
        matrix that is already on the device.  Like the reference, the max_rank largest values come
        smallest-first when max_rank < n_signals - 1 (scipy svds) and largest-first otherwise; vectors
        are unit norm with their largest component real positive (the reference's phase is arbitrary).
        """
        from . import _stage_d
        W, R, K, N, C = self._shape5
        max_rank = int(max_rank)
        if not 1 <= max_rank <= min(C, R * K):
            raise ValueError(f"max_rank must be between 1 and min(n_signals, n_trials * n_tapers) = {min(C, R * K)}")
        if C > _lib.load().sc_global_coherence_max_signals():
            raise ValueError(f"global_coherence supports n_signals <= {_lib.load().sc_global_coherence_max_signals()}")
        accum, n_obs, n_freq = self._csm_records("global", "trials_tapers")
        mem = self._memory(accum)
        values, vectors = _stage_d.global_coherence(mem, accum, W, n_freq, N, C, _lib.PLANE_CSM, self._n_observations_total(n_obs),
                                                    max_rank, ascending=max_rank < C - 1)
        return mem.download(values), mem.download(vectors)

    # ---- canonical coherence (reference connectivity.py:745-820) --------------------------
    def canonical_coherence(self, group_labels):
        """Maximal coherence between linear combinations of each pair of channel groups.

        Returns (array (n_time_windows, n_frequencies, n_groups, n_groups), sorted labels).
        Like the reference this always averages over trials and tapers.
        """
        from . import engine
        accum, n_obs, _ = self._csm_records("canonical", "trials_tapers", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        labels, groups, small = self._canonical_groups(group_labels, n_total)
        lo, hi, per = self._canonical_bins(accum.shape[0])
        n_g = len(groups)
        import torch
        if hi > lo:
            out = torch.ones((hi - lo, n_g, n_g), dtype=torch.float64, device=accum.device)
            out[:, torch.arange(n_g), torch.arange(n_g)] = float("nan")
            n_fail = 0
            if len(small) >= 2:
                sub, n_fail = engine.canonical_coherence(accum[lo:hi], self._shape5[4], _lib.PLANE_CSM, n_total,
                                                         [groups[k] for k in small])
                idx = torch.as_tensor(small, device=accum.device)
                out[:, idx[:, None], idx[None, :]] = sub
        else:                                  # more processes than bins: this one has nothing to evaluate
            out, n_fail = torch.empty((0, n_g, n_g), dtype=torch.float64, device=accum.device), 0
        out = self._canonical_gather(out, accum.shape[0], per)
        self._canonical_failed(n_fail)
        W = self._shape5[0]
        return out.cpu().numpy().reshape(W, self._n_freq, len(labels), len(labels)), labels

    def _canonical_groups(self, group_labels, n_total):
        """(np.unique of the labels, the channel indices of every group, the indices of the groups that go to the device)."""
        group_labels = np.asarray(group_labels)
        labels = np.unique(group_labels)
        groups = [np.flatnonzero(np.isin(group_labels, lab)) for lab in labels]
        # A group with at least as many channels as there are observations spans the whole observation space: the
        # orthonormal row-space basis V_g the reference gets from its thin SVD (connectivity.py:1979-2032) is then the full
        # n_obs-dimensional space, V_g^H V_h has orthonormal columns for ANY other group h, and every singular value of the
        # pair is 1 -- the canonical coherence is 1 (the reference returns 1 +- 3e-15 there: generic, full-row-rank data).
        # Such groups have no Cholesky factor (their cross-spectral block is rank deficient), so they stay out of the
        # device kernel; the pairs among the remaining groups go through the CSM form as before.
        small = [k for k, g in enumerate(groups) if len(g) < n_total]
        max_group = int(_lib.load().sc_canonical_max_group())
        if any(len(groups[k]) > max_group for k in small):
            raise ValueError(f"canonical_coherence: groups of more than {max_group} channels need n_trials * n_tapers "
                             "<= the group size (their coherence is then 1) -- the whitening kernel takes up to "
                             f"{max_group} channels per group")
        return labels, groups, small

    def canonical_coherence_vectors(self, group_labels):
        """The channel weights that attain the canonical coherence of each pair of channel groups, the topographies to plot for
        them, and every further canonical coherence of the pair.  Per frequency and pair of groups a, b of the cross-spectral
        matrix S (always averaged over trials and tapers, as ``canonical_coherence``), with rho_1 >= rho_2 >= ... the singular
        values of S_aa^-1/2 S_ab S_bb^-1/2:

        ``coherence``: rho_1 (``canonical_coherence`` returns its square, as the reference does).
        ``coherences``: every rho_k, descending; -sum_k ln(1 - rho_k^2) is ``linear_dependence().total``.
        ``filters``: the complex weights alpha (group a), beta (group b) with alpha^H S_aa alpha = beta^H S_bb beta = 1 that
        maximise alpha^H S_ab beta = rho_1 (real) -- project the data of a group onto its filter to get the coupled component.
        ``patterns``: a = S_aa alpha, b = S_bb beta -- how strongly every channel sees that component (Haufe et al. 2014): these
        are the maps to plot, not the filters.  S_ab beta = rho_1 a and S_ab^H alpha = rho_1 b.
        One joint unit phase per pair is free: the entry of largest magnitude (lowest index on a tie) of the pattern of the group
        with the lower label is real and positive (the rule of ``global_coherence``).

        Returns the named tuple (coherence, coherences, filters, patterns, labels, members): ``coherence`` float64
        [n_time_windows, n_frequencies, G, G], NaN diagonal; ``coherences`` float64 [..., G, G, n_max], NaN beyond min(n_a, n_b) and
        on the diagonal; ``filters`` and ``patterns`` complex128 [..., G, G, n_max] with entry [..., a, b, :n_a] the vector of group a
        in its pairing with group b (both orders of a pair are filled), NaN beyond n_a and on the diagonal; ``labels`` =
        np.unique(group_labels); ``members[g]`` the channel indices of group g in the order of the last axis.  Group sizes, the
        ValueError for a group that is too large and the warning for blocks that are not positive definite (NaN in every output
        of the pair) are those of ``canonical_coherence``.  A group with at least as many channels as observations has coherence 1
        with every other group: ``coherences[..., :min(n_a, n_b)]`` is 1 and the vectors are NaN (no direction is singled out).
        A pair whose cross-spectrum is exactly 0 has coherences 0 and NaN vectors (no warning).  Elsewhere the vectors are
        computed however small rho_1 is -- they mean nothing where rho_1 is not distinguishable from 0, and where rho_1 and
        rho_2 nearly coincide they are one of many equally good pairs (sc_canonical.hip).
        """
        from . import engine
        import torch
        group_labels = self._canonical_labels(group_labels)                     # (the labels are checked before any device work)
        accum, n_obs, _ = self._csm_records("canonical", "trials_tapers", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        labels, groups, small = self._canonical_groups(group_labels, n_total)
        G, n_max = len(groups), max(len(g) for g in groups)
        lo, hi, per = self._canonical_bins(accum.shape[0])
        n_part = max(hi - lo, 0)
        coherence = torch.ones((n_part, G, G), dtype=torch.float64, device=accum.device)
        coherence[:, torch.arange(G), torch.arange(G)] = float("nan")
        coherences = torch.as_tensor(self._canonical_ones(groups), device=accum.device).expand(n_part, G, G, n_max).clone()
        filters = torch.full((n_part, G, G, n_max, 2), float("nan"), dtype=torch.float64, device=accum.device)
        patterns = filters.clone()
        n_fail = 0
        if hi > lo and len(small) >= 2:
            sub_members, sub_sizes, _ = _lib.member_table([groups[k] for k in small])
            c, cs, f, p, n_fail = engine.canonical_coherence_vectors(accum[lo:hi], self._shape5[4], _lib.PLANE_CSM, n_total,
                                                                     sub_members, sub_sizes)
            idx = torch.as_tensor(small, device=accum.device)
            coherence[:, idx[:, None], idx[None, :]] = c
            coherences[:, idx[:, None], idx[None, :]] = float("nan")
            coherences[:, idx[:, None], idx[None, :], :cs.shape[-1]] = cs
            filters[:, idx[:, None], idx[None, :], :f.shape[-2]] = f
            patterns[:, idx[:, None], idx[None, :], :p.shape[-2]] = p
        parts = [self._canonical_gather(t, accum.shape[0], per) for t in (coherence, coherences, filters, patterns)]
        self._canonical_failed(n_fail)
        return self._canonical_vectors_result([engine.to_host(t) for t in parts], labels, groups)

    def _canonical_labels(self, group_labels):
        group_labels = np.asarray(group_labels)
        if group_labels.shape != (self._shape5[4],):
            raise ValueError(f"canonical_coherence_vectors: group_labels needs one label per signal ({self._shape5[4]}), got shape "
                             f"{group_labels.shape}")
        return group_labels

    @staticmethod
    def _canonical_ones(groups):
        """coherences before the device fills the pairs it evaluates [G, G, n_max]: 1 up to min(n_a, n_b) (every canonical
        coherence of a pair with a group that spans the observation space is 1), NaN beyond and on the diagonal."""
        G, n_max = len(groups), max(len(g) for g in groups)
        ones = np.full((G, G, n_max), np.nan)
        for a in range(G):
            for b in range(G):
                if a != b:
                    ones[a, b, :min(len(groups[a]), len(groups[b]))] = 1.0
        return ones

    def _canonical_vectors_result(self, host, labels, groups):
        """The named tuple from the four host arrays [n_bins, G, G(, n_max(, 2))]: (re, im) pairs become complex128."""
        coherence, coherences, filters, patterns = (np.ascontiguousarray(t) for t in host)
        G, n_max = len(groups), coherences.shape[-1]
        shape = (self._shape5[0], self._n_freq, G, G)
        return CanonicalVectors(coherence.reshape(shape), coherences.reshape(shape + (n_max,)),
                                filters.view(np.complex128).reshape(shape + (n_max,)),
                                patterns.view(np.complex128).reshape(shape + (n_max,)), labels,
                                [np.asarray(g, dtype=np.int64) for g in groups])

    def _canonical_failed(self, n_fail):
        if n_fail:
            logger.warning(f"{n_fail} group cross-spectral blocks were not positive definite (NaN output)")

    def _canonical_bins(self, n_bins):
        """Bins [lo, hi) this process evaluates and the per-process count (all of them here; 1/N of them in
        parallel.ShardedConnectivity)."""
        return 0, n_bins, n_bins

    def _canonical_gather(self, part, n_bins, per):
        return part

    # ---- multivariate imaginary coherence (Ewald, Marzetti, Zappasodi, Meinecke & Nolte 2012) ----------------
    def maximized_imaginary_coherence(self, group_labels):
        """Maximized imaginary coherence (MIC) between each pair of channel groups: the largest singular value of
        (Re S_aa)^-1/2 Im S_ab (Re S_bb)^-1/2, in [0, 1].  Like imaginary_coherence, instantaneous mixing (volume conduction,
        source leakage) cannot create it: it is 0 wherever the cross-spectrum is real, and real invertible mixing inside a group
        leaves it unchanged.  With one channel per group it is |imaginary_coherence()|.

        Returns (array [kept axes..., n_frequencies, n_groups, n_groups] float64, symmetric with a NaN diagonal,
        np.unique(group_labels)); the expectation is the object's ``expectation_type``.  Groups of up to
        sc_canonical_max_group() = 128 channels (sc_canonical.hip).  A group of more than 2 n_observations channels has a
        singular real block: its pairs are NaN (one warning counts the groups), as are the pairs with a block the device
        reports not positive definite (one warning).
        """
        mic, _, labels = self._imaginary_interaction(group_labels)
        return mic, labels

    def multivariate_interaction_measure(self, group_labels):
        """Multivariate interaction measure (MIM) between each pair of channel groups: the sum of the squared singular values of
        (Re S_aa)^-1/2 Im S_ab (Re S_bb)^-1/2 = tr((Re S_aa)^-1 Im S_ab (Re S_bb)^-1 Im S_ab^T), in [0, min(n_a, n_b)];
        MIC^2 <= MIM <= min(n_a, n_b) MIC^2.  Returns, computes and limits as maximized_imaginary_coherence (one device call
        gives both)."""
        _, mim, labels = self._imaginary_interaction(group_labels)
        return mim, labels

    def _interaction_groups(self, group_labels):
        return _lib.interaction_groups(group_labels, self._shape5[4], int(_lib.load().sc_canonical_max_group()))

    def _interaction_kept(self, sizes, n_obs_total):
        keep, n_out = _lib.interaction_kept(sizes, n_obs_total)
        if n_out:
            logger.warning(f"imaginary interaction: {n_out} groups have more channels than twice the {n_obs_total} observations "
                           "(singular real cross-spectral blocks): NaN")
        return keep

    def _interaction_failed(self, n_fail):
        if n_fail:
            logger.warning(f"imaginary interaction: {n_fail} group pairs have a real cross-spectral block that is not positive "
                           "definite (NaN output)")

    def _imaginary_interaction(self, group_labels):
        from . import engine
        import torch
        labels, members, sizes, _ = self._interaction_groups(group_labels)      # (the labels are checked before any device work)
        accum, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        keep = self._interaction_kept(sizes, n_total)
        G = len(labels)
        lo, hi, per = self._canonical_bins(accum.shape[0])
        mic = torch.full((max(hi - lo, 0), G, G), float("nan"), dtype=torch.float64, device=accum.device)
        mim = mic.clone()
        n_fail = 0
        if hi > lo and len(keep) >= 2:
            sub_members, sub_sizes, _ = _lib.member_table([members[k, :sizes[k]] for k in keep])
            a, b, n_fail = engine.imaginary_interaction(accum[lo:hi], self._shape5[4], _lib.PLANE_CSM, n_total, sub_members,
                                                        sub_sizes)
            idx = torch.as_tensor(keep, device=accum.device)
            mic[:, idx[:, None], idx[None, :]] = a
            mim[:, idx[:, None], idx[None, :]] = b
        mic = self._canonical_gather(mic, accum.shape[0], per)
        mim = self._canonical_gather(mim, accum.shape[0], per)
        self._interaction_failed(n_fail)
        shape = self._kept_shape() + (self._n_freq, G, G)
        return engine.to_host(mic).reshape(shape), engine.to_host(mim).reshape(shape), labels

    def maximized_imaginary_coherence_vectors(self, group_labels):
        """The channel weights that attain ``maximized_imaginary_coherence`` and the topographies to plot for them (MNE-Connectivity's
        ``patterns`` of ``mic``).  Per frequency and pair of groups a, b with R_g = Re S_gg and I = Im S_ab:

        ``filters``: the weights alpha (group a), beta (group b) with alpha^T R_a alpha = beta^T R_b beta = 1 that maximise
        alpha^T I beta = MIC -- Ewald's R^-1/2 u; project the data of a group onto its filter to get the interacting component.
        ``patterns``: a = R_a alpha, b = R_b beta -- how strongly every channel sees that component (Haufe et al. 2014): these are
        the maps to plot, not the filters.  I beta = MIC a and I^T alpha = MIC b.
        One joint sign per pair is free: the entry of largest magnitude (lowest index on a tie) of the pattern of the group with
        the lower label is positive.

        Returns the named tuple (mic, filters, patterns, labels, members): ``mic`` [kept axes..., n_frequencies, G, G] as
        maximized_imaginary_coherence; ``filters`` and ``patterns`` float64 [kept axes..., n_frequencies, G, G, n_max] with
        entry [..., a, b, :n_a] the vector of group a in its interaction with group b (both orders of a pair are filled), NaN
        beyond n_a and on the diagonal; ``labels`` = np.unique(group_labels); ``members[g]`` the channel indices of group g in the
        order of the last axis.  Expectation, group sizes, rank rule and warnings of maximized_imaginary_coherence: a pair whose
        MIC is NaN has NaN vectors.  A pair whose cross-spectrum is exactly real has MIC 0 and NaN vectors (no direction is
        singled out; no warning).  Elsewhere the vectors are computed however small MIC is -- they mean nothing where MIC is not
        distinguishable from 0, and where the two largest singular values nearly coincide they are one of many equally good
        pairs (sc_canonical.hip).
        """
        from . import engine
        import torch
        labels, members, sizes, _ = self._interaction_groups(group_labels)      # (the labels are checked before any device work)
        accum, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        keep = self._interaction_kept(sizes, n_total)
        G, n_max = len(labels), int(sizes.max())
        lo, hi, per = self._canonical_bins(accum.shape[0])
        mic = torch.full((max(hi - lo, 0), G, G), float("nan"), dtype=torch.float64, device=accum.device)
        filters = torch.full((max(hi - lo, 0), G, G, n_max), float("nan"), dtype=torch.float64, device=accum.device)
        patterns = filters.clone()
        n_fail = 0
        if hi > lo and len(keep) >= 2:
            sub_members, sub_sizes, _ = _lib.member_table([members[k, :sizes[k]] for k in keep])
            a, f, p, n_fail = engine.imaginary_interaction_vectors(accum[lo:hi], self._shape5[4], _lib.PLANE_CSM, n_total,
                                                                   sub_members, sub_sizes)
            idx = torch.as_tensor(keep, device=accum.device)
            mic[:, idx[:, None], idx[None, :]] = a
            filters[:, idx[:, None], idx[None, :], :f.shape[-1]] = f
            patterns[:, idx[:, None], idx[None, :], :p.shape[-1]] = p
        mic = self._canonical_gather(mic, accum.shape[0], per)
        filters = self._canonical_gather(filters, accum.shape[0], per)
        patterns = self._canonical_gather(patterns, accum.shape[0], per)
        self._interaction_failed(n_fail)
        shape = self._kept_shape() + (self._n_freq, G, G)
        return InteractionVectors(engine.to_host(mic).reshape(shape), engine.to_host(filters).reshape(shape + (n_max,)),
                                  engine.to_host(patterns).reshape(shape + (n_max,)), labels,
                                  [members[g, :sizes[g]].astype(np.int64) for g in range(G)])

    # ---- total, instantaneous and lagged linear dependence (Pascual-Marqui 2007, arXiv:0706.1776) -----------------
    def linear_dependence(self, group_labels=None):
        """Pascual-Marqui's decomposition of the linear dependence between each pair of signal groups a, b (J their union) into an
        instantaneous (zero-lag) and a lagged part, per frequency, with S the cross-spectral matrix:

        ``total``          ln det S_aa + ln det S_bb - ln det S_JJ = -sum_k ln(1 - rho_k^2) over the canonical coherences
        ``instantaneous``  the same of Re S
        ``lagged``         total - instantaneous: 0 wherever the cross-spectrum is real, so instantaneous mixing (volume
                           conduction, source leakage) cannot create it

        All are >= 0 and unchanged by real invertible mixing inside a group (the total also by complex mixing); Pascual-Marqui's
        coherences are 1 - exp(-F).  ``group_labels`` None: every signal is its own group (``lagged_coherence`` gives the
        pairwise lagged coherence directly).

        Returns the named tuple (total, instantaneous, lagged, labels): float64 arrays [kept axes..., n_frequencies, G, G],
        symmetric with a NaN diagonal, over the object's ``expectation_type``; ``labels`` = np.unique(group_labels) (np.arange of
        the signals without labels).  A pair of groups may have up to sc_linear_dependence_max_joint() = 128 signals together
        (ValueError beyond, naming the pair; single signals: any number).  A pair with more signals than observations has a
        singular joint matrix: NaN (one warning counts the pairs), as is a (frequency, pair) whose matrices the device cannot
        factorise -- a signal without power, or not positive definite to rounding (one warning counts them).  sc_dependence.hip,
        DESIGN 4.15.
        """
        out, labels = self._linear_dependence(group_labels, ("total", "instantaneous", "lagged"))
        return LinearDependence(out["total"], out["instantaneous"], out["lagged"], labels)

    def lagged_coherence(self):
        """Lagged coherence of each pair of signals (Pascual-Marqui 2007; LORETA-KEY, FieldTrip): the squared quantity
        rho^2_lag = (Im c)^2 / (1 - (Re c)^2) of the coherency c, = 1 - exp(-F_lagged) of ``linear_dependence()``; in [0, 1], 0
        wherever the cross-spectrum is real.  float64 [kept axes..., n_frequencies, n_signals, n_signals], symmetric with a NaN
        diagonal.  NaN entries and warnings as ``linear_dependence``."""
        out, _ = self._linear_dependence(None, ("lagged",))
        return -np.expm1(-out["lagged"])

    def _dependence_groups(self, group_labels):
        return _lib.dependence_groups(group_labels, self._shape5[4], int(_lib.load().sc_linear_dependence_max_joint()))

    def _dependence_warnings(self, sizes, n_total, n_fail):
        n_skipped = _lib.dependence_rank_skipped(sizes, n_total)
        if n_skipped:
            logger.warning(f"linear dependence: {n_skipped} group pairs have more signals together than the {n_total} observations "
                           "(singular joint cross-spectral matrix): NaN")
        if n_fail:
            logger.warning(f"linear dependence: {n_fail} (frequency, pair) problems have a signal without power or a cross-spectral "
                           "matrix that is not positive definite to rounding (NaN output)")

    def _linear_dependence(self, group_labels, want):
        """({name: [kept axes..., n_frequencies, G, G] float64} for the names of ``want``, labels)."""
        from . import engine
        import torch
        labels, members, sizes, _ = self._dependence_groups(group_labels)       # (the labels are checked before any device work)
        accum, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        G = len(labels)
        lo, hi, per = self._canonical_bins(accum.shape[0])
        n_fail = 0
        if hi > lo:
            res, n_fail = engine.linear_dependence(accum[lo:hi], self._shape5[4], _lib.PLANE_CSM, n_total, members, sizes, want)
        else:                                  # more processes than bins: this one has nothing to evaluate
            res = {name: torch.empty((0, G, G), dtype=torch.float64, device=accum.device) for name in want}
        self._dependence_warnings(sizes, n_total, n_fail)
        shape = self._kept_shape() + (self._n_freq, G, G)
        return {name: engine.to_host(self._canonical_gather(res[name], accum.shape[0], per)).reshape(shape) for name in want}, labels

    # ---- partial and multiple coherence (Bendat & Piersol 1986, ch. 7; Dahlhaus 2000) ----------------------------
    def partial_coherency(self, given=None, signals=None):
        """Coherency of each pair of signals after the linear influence of other signals is removed from both.

        Without keywords ALL other signals are removed: -G_ij / sqrt(G_ii G_jj) with G the inverse of the cross-spectral matrix.
        Where two signals are coherent only because both see a third recorded signal, it is 0 while ``coherency()`` is not; with
        two signals it is ``coherency()``.  Returns complex128 [kept axes..., n_frequencies, n_signals, n_signals], Hermitian with
        a NaN diagonal; the expectation is the object's ``expectation_type``.  Up to sc_partial_coherence_max_signals() = 128
        signals (sc_partial.hip; ValueError beyond).  The cross-spectral matrix of fewer observations than signals is singular:
        everything is NaN (one warning, no device work); a matrix the device cannot invert -- a channel without power, two
        identical channels, a condition number beyond 1 / (n_signals 2^-52) after scaling to a unit diagonal -- gives NaN in its
        bin (one warning counts them).  No bias correction.

        ``given``: the indices of the m signals to remove (EOG, ECG, a reference sensor, a stimulus trace; FieldTrip's
        ``partchannel``), and ``signals`` the indices of the a signals to keep -- by default every signal that is not given,
        ascending.  The result is E_ij / sqrt(E_ii E_jj) with E = S_AA - S_AZ S_ZZ^-1 S_ZA the cross-spectrum of what is left of
        the kept signals A after each is regressed on the given signals Z, complex128 [kept axes..., n_frequencies, a, a] in the
        order of ``signals``.  The record may then have any number of signals: 1 <= m <= 128, 1 <= a <= 1024 and
        sc_partial_given_lds_bytes(a, m) within 160 KB (1024 kept given 8, 512 given 16, 300 given 6, every a + m <= 128);
        ValueError with the numbers beyond, and for lists that are empty, overlap, repeat a signal or leave the range.  No more
        observations than given signals leave no residual: everything is NaN (one warning, no device work).  A bin whose given
        block cannot be factored (a given signal without power, two identical given signals) is NaN (one warning counts the
        bins); a kept signal the given ones explain entirely (a copy of one) is NaN in its row and column of its bin, nothing
        else (one warning counts the cases).
        """
        return self._partial_dispatch("coherency", given, signals)

    def partial_coherence_magnitude(self, given=None, signals=None):
        """|partial_coherency(given, signals)|, in [0, 1] and not squared: float64 shaped like it, symmetric with a NaN diagonal.
        Computes and limits as partial_coherency."""
        return self._partial_dispatch("magnitude", given, signals)

    def multiple_coherence_magnitude(self, given=None, signals=None):
        """The share of each signal's power that other signals explain linearly, as a magnitude.  Without keywords the share that
        ALL the other signals explain: sqrt(1 - 1 / (S_ii G_ii)) in [0, 1), float64 [kept axes..., n_frequencies, n_signals].
        With ``given`` it is the share of the power of each kept signal that the GIVEN signals explain -- not all the others --,
        sqrt(1 - E_ii / S_ii) in [0, 1], float64 [kept axes..., n_frequencies, a] in the order of ``signals``; exactly 1 for a
        kept signal that the given ones explain entirely.  Computes and limits as partial_coherency."""
        return self._partial_dispatch("multiple", given, signals)

    def _partial_dispatch(self, name, given, signals):
        if given is None and signals is None:
            return self._partial_coherence(name)
        return self._partial_coherence_given(name, given, signals)

    def _partial_given_request(self, name, given, signals):
        """(kept, given int32 index arrays, the signal axes, the whole shape, the dtype) of the output ``name`` of
        sc_partial_coherence_given_f64, after every check that needs no device."""
        kept, z = _lib.partial_given_indices(given, signals, self._shape5[4])
        lib = _lib.load()
        a, m = len(kept), len(z)
        max_kept, max_given = int(lib.sc_partial_given_max_kept()), int(lib.sc_partial_given_max_given())
        if m > max_given or a > max_kept:
            raise ValueError(f"partial coherence given a set takes at most {max_given} given and {max_kept} kept signals "
                             f"(got {m} given, {a} kept)")
        need, limit = int(lib.sc_partial_given_lds_bytes(a, m)), int(lib.sc_partial_given_lds_limit())
        if need > limit:
            raise ValueError(f"partial coherence of {a} kept signals given {m} needs {need} bytes of LDS, beyond the {limit} of a "
                             "compute unit: keep or give fewer signals")
        tail = (a,) if name == "multiple" else (a, a)
        return kept, z, tail, self._kept_shape() + (self._n_freq,) + tail, np.complex128 if name == "coherency" else np.float64

    def _partial_given_few_observations(self, n_total, m):
        if n_total <= m:
            logger.warning(f"partial coherence: {m} given signals from {n_total} observations leave no residual (no more "
                           "observations than given signals): NaN")
        return n_total <= m

    def _partial_given_failed(self, counts):
        n_failed, n_explained = counts
        if n_failed:
            logger.warning(f"partial coherence: {n_failed} matrices of the given signals have no inverse (a signal without power, "
                           "or not positive definite to rounding): NaN output")
        if n_explained:
            logger.warning(f"partial coherence: {n_explained} (bin, signal) cases where the given signals explain a kept signal "
                           "entirely: NaN in its pairs")

    def _partial_coherence_given(self, name, given, signals):
        from . import engine
        import torch
        kept, z, tail, shape, dtype = self._partial_given_request(name, given, signals)
        accum, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        if self._partial_given_few_observations(n_total, len(z)):
            return np.full(shape, np.nan, dtype=dtype)
        lo, hi, per = self._canonical_bins(accum.shape[0])
        counts = (0, 0)
        if hi > lo:
            res, counts = engine.partial_coherence_given(accum[lo:hi], self._shape5[4], _lib.PLANE_CSM, n_total, kept, z, (name,))
            out = res[name]
        else:                                  # more processes than bins: this one has nothing to evaluate
            out = torch.empty((0,) + tail, dtype=engine._TORCH_DTYPES[dtype], device=accum.device)
        if name == "coherency":                # (gathered as pairs of doubles: not every backend moves complex tensors)
            out = torch.view_as_complex(self._canonical_gather(torch.view_as_real(out), accum.shape[0], per).contiguous())
        else:
            out = self._canonical_gather(out, accum.shape[0], per)
        self._partial_given_failed(counts)
        return engine.to_host(out).reshape(shape)

    def _partial_shape(self, name):
        """(n_signals after the range check, the signal axes, the whole shape, the dtype) of the output ``name`` of
        sc_partial_coherence_f64."""
        C = self._shape5[4]
        limit = int(_lib.load().sc_partial_coherence_max_signals())
        if not 2 <= C <= limit:
            raise ValueError(f"partial and multiple coherence take between 2 and {limit} signals (got {C})")
        tail = (C,) if name == "multiple" else (C, C)
        return C, tail, self._kept_shape() + (self._n_freq,) + tail, np.complex128 if name == "coherency" else np.float64

    def _partial_few_observations(self, n_total, C):
        if n_total < C:
            logger.warning(f"partial coherence: the cross-spectral matrix of {C} signals from {n_total} observations is singular "
                           "(fewer observations than signals): NaN")
        return n_total < C

    def _partial_failed(self, n_fail):
        if n_fail:
            logger.warning(f"partial coherence: {n_fail} cross-spectral matrices have no inverse (a channel without power, or not "
                           "positive definite to rounding): NaN output")

    def _partial_coherence(self, name):
        from . import engine
        import torch
        C, tail, shape, dtype = self._partial_shape(name)
        accum, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        if self._partial_few_observations(n_total, C):
            return np.full(shape, np.nan, dtype=dtype)
        lo, hi, per = self._canonical_bins(accum.shape[0])
        n_fail = 0
        if hi > lo:
            res, n_fail = engine.partial_coherence(accum[lo:hi], C, _lib.PLANE_CSM, n_total, (name,))
            out = res[name]
        else:                                  # more processes than bins: this one has nothing to evaluate
            out = torch.empty((0,) + tail, dtype=engine._TORCH_DTYPES[dtype], device=accum.device)
        if name == "coherency":                # (gathered as pairs of doubles: not every backend moves complex tensors)
            out = torch.view_as_complex(self._canonical_gather(torch.view_as_real(out), accum.shape[0], per).contiguous())
        else:
            out = self._canonical_gather(out, accum.shape[0], per)
        self._partial_failed(n_fail)
        return engine.to_host(out).reshape(shape)

    # ---- delete-one jackknife standard errors (Thomson & Chave 1991; Chronux err = [2 p]) --------------------
    def jackknife(self, measures=("coherence_magnitude",), over="trials"):
        """Delete-one jackknife of power and coherence on their variance-stabilising scales: standard errors that rest on the data
        (overlapping windows, non-stationary trials) instead of the closed forms of ``statistics``.

        ``measures``: any of "power" (theta = ln power, transform "log"), "coherence_magnitude" (theta = arctanh |coherency|,
        "fisher_z"; ``coherence_magnitude()`` itself is the squared magnitude, tanh(theta)^2) and "imaginary_coherence" (signed, "identity": its absolute value at the full estimate is
        ``imaginary_coherence()``); all of them come from ONE pass over the spectra (sc_jackknife.hip).  ``over="trials"``: a
        delete unit is everything one trial contributes to the expectation (needs an ``expectation_type`` that averages over
        trials and n_trials >= 2); ``over="observations"``: every averaged observation is a unit (the Chronux choice; any
        ``expectation_type``, n_observations >= 2).  Leaving a unit out is S - G_u with G_u the unit's own cross-spectrum.

        Returns {name: statistics.JackknifeResult}: ``estimate``, ``bias_corrected`` and ``standard_error`` are float64 arrays
        shaped like the measure's own output ([kept axes..., n_frequencies, n_signals] for power, [..., n_signals, n_signals] with
        a NaN diagonal otherwise; the imaginary coherence is antisymmetric); ``statistics.jackknife_confidence_intervals`` turns
        one into an interval on the natural scale.  A channel without power in a bin gives NaN in its entries (one warning counts
        them).  The coherence magnitude is formed as |S_ij| (1 / sqrt S_ii) (1 / sqrt S_jj); where it is 1 up to rounding (two
        identical channels; a leave-one-out estimate of a single observation, which also warns) the pair's ``estimate`` is
        arctanh of a number within a few ulp of 1 -- at least 17, inf, or NaN beyond 1 -- and its other two outputs carry no
        promise (the float64 reference rounds differently there); no other entry is affected.  ValueError for an
        unknown or empty measure list, a bad ``over`` and fewer than two units, before any device work.

        The phase-lag family, on the identity scale and signed where the measure is signed: "phase_lag_index",
        "weighted_phase_lag_index" (both antisymmetric), "debiased_squared_phase_lag_index" and
        "debiased_squared_weighted_phase_lag_index" (symmetric; NaN where sum |Im s|^2 = sum (Im s)^2 exactly, as at the zero and
        Nyquist bins of a real series) -- the jackknife of FieldTrip's ft_connectivity_wpli.  They come from a pass of their own
        (jk_phase_kernel) against totals that one more pass sums from the same spectra in fp64 (kept for the next request);
        ``estimate`` equals the method's value off the NaN diagonal to the engine's precision.  The two debiased measures need
        two observations in a delete-one set (ValueError for two units of one observation).  The results are ordered: the three
        measures above first, then these four.
        """
        old, new = _lib.jackknife_split(measures)
        # (every request is checked before any device work)
        plan = _lib.jackknife_request(old, over, self.expectation_type, self._jackknife_trials(), self.n_observations) if old else None
        phase_plan = (_lib.jackknife_phase_request(new, over, self.expectation_type, self._jackknife_trials(), self.n_observations)
                      if new else None)
        out = {}
        if plan is not None:
            out.update(self._jackknife_first_family(plan, over))
        if phase_plan is not None:
            out.update(self._jackknife_phase_family(phase_plan, over))
        return out

    def _jackknife_results(self, flat, n_bins, names, table, n_units, over):
        """{name: JackknifeResult} from the library's flat output (_lib.jackknife_blocks) for the measures ``names`` of ``table``."""
        from .statistics import JackknifeResult, jackknife_finish
        blocks, _ = _lib.jackknife_blocks(names, n_bins, self._shape5[4])
        out = {}
        for name, at, size, shape in blocks:
            theta, s1, s2 = (flat[at + k * size:at + (k + 1) * size].reshape(self._kept_shape() + (self._n_freq,) + shape[1:])
                             for k in range(3))
            est, corrected, se = jackknife_finish(theta, s1, s2, n_units)
            out[name] = JackknifeResult(est, corrected, se, table[name][1], n_units, over)
        return out

    def _jackknife_first_family(self, plan, over):
        """Power, coherence magnitude and imaginary coherence: jk_kernel against the CSM record."""
        names, mask, over_id, n_units = plan
        if n_units == 2 and self.n_observations == 2 and "coherence_magnitude" in names:
            logger.warning("jackknife: with two delete units of one observation each a leave-one-out estimate is a single observation, "
                           "whose coherence magnitude is identically 1: the coherence_magnitude results are inf, NaN or rounding noise")
        flat, n_bins = self._jackknife_sums(mask, over_id, n_units)
        out = self._jackknife_results(flat, n_bins, names, _lib.JACKKNIFE_MEASURES, n_units, over)
        first = out[names[0]].estimate
        n_nan = int(np.isnan(first).sum())
        if names[0] != "power":
            n_nan -= first.size // first.shape[-1]          # (the diagonal is NaN by definition)
        if n_nan:
            logger.warning(f"jackknife: {n_nan} entries of {names[0]} are NaN (a channel without power in a bin)")
        return out

    def _jackknife_phase_family(self, plan, over):
        """The phase-lag family: jk_phase_kernel against a record of totals with the planes its measures read."""
        names, mask, over_id, n_units, planes = plan
        flat, n_bins = self._jackknife_phase_sums(mask, planes, over_id, n_units)
        out = self._jackknife_results(flat, n_bins, names, _lib.JACKKNIFE_PHASE_MEASURES, n_units, over)
        nan = np.isnan(out[names[0]].estimate)
        C = nan.shape[-1]
        nan[..., np.arange(C), np.arange(C)] = False        # (the diagonal is NaN by definition)
        if names[0] == "debiased_squared_weighted_phase_lag_index" and self._device().real_input:
            # a real series has Im s = 0 in every observation at the zero bin and at the Nyquist bin of an even length: the
            # denominator sum |Im s|^2 - sum (Im s)^2 is exactly 0 there and the measure NaN by its definition
            nan[..., 0, :, :] = False
            if self._shape5[3] % 2 == 0:
                nan[..., -1, :, :] = False
        n_nan = int(nan.sum())
        if n_nan:
            logger.warning(f"jackknife: {n_nan} entries of {names[0]} are NaN (coefficients that are not finite, or a pair whose "
                           "sum |Im s|^2 equals its sum (Im s)^2)")
        return out

    def _jackknife_trials(self):
        """Trials of the whole job (parallel.ShardedConnectivity: over every rank)."""
        return int(self._shape5[1])

    def _jackknife_sums(self, mask, over_id, n_units):
        """(the library's output as a flat float64 NumPy array -- _lib.jackknife_blocks --, n_bins).  The spectra are asked for
        without a planes hint (the kernel reads complex64 / complex128; spectra already held as f16 pieces are decoded once);
        the total is the CSM record of every rank's trials -- the one MIC / MIM read, cached under the same key."""
        from . import _stage_d
        accum, _, _ = self._csm_records("interaction", two_sided=False)
        mem = self._memory(accum)
        out, n_bins = _stage_d.jackknife(mem, self._device(), self.expectation_type, accum, _lib.PLANE_CSM, mask, over_id, n_units,
                                         n_freq=self._n_freq)
        return mem.download(self._jackknife_reduce(out, mask, n_bins)), n_bins

    def _jackknife_phase_sums(self, mask, planes, over_id, n_units):
        """_jackknife_sums for the phase-lag family.  The spectra are asked for without a planes hint, as there.  The total is a
        record of doubles with the families ``planes`` that the jackknife sums from the spectra itself
        (_stage_d.jackknife_phase_totals: the fp64 sum of exactly the unit sums the kernel subtracts, on both engines), summed
        over every rank's trials and cached like the measures' own records; a later request over the same units that needs no
        other plane reads it again."""
        from . import _stage_d
        sp = self._device()
        mem = self._memory(sp)
        mine = [k for k in self._accum_cache if isinstance(k, tuple) and k[0] == "jackknife_phase" and k[2] == over_id]
        have = next((k for k in mine if k[1] & planes == planes), None)
        if have is None:
            total, n_obs = _stage_d.jackknife_phase_totals(mem, sp, self.expectation_type, planes, over_id, n_freq=self._n_freq)
            for old in [k for k in mine if k[1] & planes == k[1]]:
                del self._accum_cache[old]             # a record the new one covers: its memory can go
            have = ("jackknife_phase", planes, over_id)  # (the unit sums behind a total are those of this `over`)
            self._accum_cache[have] = (self._reduce_over_ranks(total), n_obs)
        out, n_bins = _stage_d.jackknife_phase(mem, sp, self.expectation_type, self._accum_cache[have][0], have[1], mask, over_id,
                                               n_units, n_freq=self._n_freq)
        return mem.download(self._jackknife_reduce(out, mask, n_bins, _lib.JACKKNIFE_PHASE_MEASURES)), n_bins

    def _jackknife_reduce(self, out, mask, n_bins, table=None):
        """Sum of the partial sums over the processes that hold the trials (nothing to add here).  ``table``: the measures the
        mask ``mask`` is of (default _lib.JACKKNIFE_MEASURES)."""
        return out

    # ---- seed-based connectivity: a few signals against a list of signals (sc_seed.hip) --------------------------------------
    def seed_connectivity(self, seeds, targets=None, measures=("coherence_magnitude",)):
        """The expectation-type measures of a few reference signals (an EMG or ECG lead, a stimulus sensor, a seed LFP) against a
        list of signals -- MNE-Connectivity's ``indices=(seeds, targets)``, FieldTrip's ``channelcmb`` -- without the all-pairs
        matrix: n_seeds x n_targets products per observation instead of n_signals^2 / 2, and ONE pass over the spectra whatever the
        measures (the all-pairs methods take one per accumulator family).

        ``seeds``: distinct signal indices in [0, n_signals), at most ``sc_seed_connectivity_max_seeds()`` (64).  ``targets``:
        distinct signal indices in any order, or None for every signal in order; seeds may be among them.  ``measures``: any
        non-empty subset, without repeats, of "coherency", "coherence_magnitude", "coherence_phase", "imaginary_coherence",
        "phase_locking_value", "pairwise_phase_consistency", "phase_lag_index", "weighted_phase_lag_index",
        "debiased_squared_phase_lag_index" and "debiased_squared_weighted_phase_lag_index".

        Returns ``SeedConnectivity(values, seeds, targets)``: ``values[name]`` has the shape [kept axes..., n_frequencies, n_seeds,
        n_targets] and the dtype of the method of that name, and ``values[name][..., s, t]`` is what
        ``getattr(self, name)()[..., seeds[s], targets[t]]`` returns: the cross-spectrum is x_seed conj(x_target), so the
        antisymmetric measures have the sign of that entry, and where a seed is its own target the entry is the method's diagonal
        (NaN for the coherency family, Im s forced to 0 for the phase-lag family); a coherence phase of a real negative
        cross-spectrum is +pi or -pi as in the method (above or below the diagonal).  ValueError, before any device work, for an
        unknown, empty or repeated measure, an empty list, an index that is out of range, not an integer or repeated, and too
        many seeds.  The float32 engine's amplitude guard applies as for the methods (section 4.3.1 of DESIGN.md)."""
        C = int(self._shape5[4])
        seeds, targets, names, codes, planes = _lib.seed_request(seeds, targets, measures, C,
                                                                 int(_lib.load().sc_seed_connectivity_max_seeds()))
        sp = self._seed_spectra(planes & ~_lib.SEED_PLANE_POWER)
        from . import _stage_d
        mem = self._memory(sp.X)
        outs = _stage_d.seed_connectivity(mem, sp, self.expectation_type, seeds, targets, planes, codes,
                                          [self._wide_output(code) for code in codes], n_freq=self._n_freq,
                                          reduce=self._reduce_over_ranks, n_observations=self._n_observations_total)
        targets = np.arange(C, dtype=np.int32) if targets is None else targets
        shape = self._kept_shape() + (self._n_freq, len(seeds), len(targets))
        return SeedConnectivity({name: mem.download(out).reshape(shape) for name, out in zip(names, outs)}, seeds, targets)

    def _seed_spectra(self, planes, method="seed_connectivity"):
        """The complex64 / complex128 spectra seed_connectivity and seed_jackknife (``method``: who asks, for a refusal's text) read: asked for without a planes hint (the kernel reads
        coefficients; spectra already held as f16 pieces are decoded once), and their complex128 copy where (Im s)^2 or s / |s| of
        this request would leave the float32 range (_guard_spectra, as _accumulators applies it)."""
        return self._guard_spectra(self._device(), planes)

    # ---- delete-one jackknife of seed-based connectivity (sc_seed_jackknife.hip) -----------------------------------------------
    def seed_jackknife(self, seeds, targets=None, measures=("coherence_magnitude",), over="trials"):
        """Delete-one jackknife standard errors of a few signals against a list of signals -- cortico-muscular or seed-to-sensor
        coherence with confidence limits (Chronux coherencyc with err = [2 p], FieldTrip's jackknife of ft_connectivity_wpli) --
        without the all-pairs jackknife's three [n_frequencies, n_signals, n_signals] arrays per measure: n_seeds x n_targets
        entries per delete unit instead of n_signals^2 / 2.

        ``seeds``, ``targets``: the rules of ``seed_connectivity``.  ``over``: the rules of ``jackknife``.  ``measures``: a
        non-empty subset, without repeats, of the six pair measures of ``jackknife`` on its scales -- "coherence_magnitude"
        (Fisher z of |coherency|), "imaginary_coherence" (signed), "phase_lag_index", "weighted_phase_lag_index",
        "debiased_squared_phase_lag_index", "debiased_squared_weighted_phase_lag_index" (identity); all of them come from ONE walk
        over the spectra, against totals that one more walk sums from the same spectra in fp64 (kept for the next request with
        the same seeds, targets and ``over``).

        Returns ``SeedJackknife(results, seeds, targets)``: ``results[name]`` is a ``statistics.JackknifeResult`` whose
        ``estimate``, ``bias_corrected`` and ``standard_error`` are float64 arrays [kept axes..., n_frequencies, n_seeds,
        n_targets], ordered as ``jackknife`` orders them; entry [..., s, t] is what ``self.jackknife((name,), over)[name]`` has at
        [..., seeds[s], targets[t]]: the cross-spectrum is x_seed conj(x_target), so the antisymmetric measures carry the sign of
        that entry, and where a seed is its own target all three are NaN.  Off those entries ``estimate`` is
        ``seed_connectivity``'s value of the same name on the statistic's scale (arctanh(sqrt(value)) for the coherence
        magnitude).  The warnings are those of ``jackknife``, counted over these entries.  ValueError, before any device work,
        for what ``seed_connectivity`` and ``jackknife`` refuse, for "power" and for a repeated measure."""
        from .statistics import JackknifeResult, jackknife_finish
        C = int(self._shape5[4])
        seeds, targets, names, mask, planes, over_id, n_units = _lib.seed_jackknife_request(
            seeds, targets, measures, over, self.expectation_type, self._jackknife_trials(), self.n_observations, C,
            int(_lib.load().sc_seed_connectivity_max_seeds()))
        if n_units == 2 and self.n_observations == 2 and "coherence_magnitude" in names:
            logger.warning("jackknife: with two delete units of one observation each a leave-one-out estimate is a single observation, "
                           "whose coherence magnitude is identically 1: the coherence_magnitude results are inf, NaN or rounding noise")
        flat, n_bins = self._seed_jackknife_sums(seeds, targets, mask, planes, over_id, n_units)
        all_targets = np.arange(C, dtype=np.int32) if targets is None else targets
        shape = self._kept_shape() + (self._n_freq, len(seeds), len(all_targets))
        size = n_bins * len(seeds) * len(all_targets)
        own = seeds[:, None] == all_targets[None, :]                # a seed that is its own target: NaN by definition
        results = {}
        for k, name in enumerate(names):
            theta, s1, s2 = (flat[(3 * k + j) * size:(3 * k + j + 1) * size].reshape(shape) for j in range(3))
            results[name] = JackknifeResult(*jackknife_finish(theta, s1, s2, n_units), _lib.SEED_JACKKNIFE_MEASURES[name][1], n_units, over)
        # one count per family, on its first measure, as jackknife does
        first = next((k for k in names if k in _lib.JACKKNIFE_MEASURES), None)
        if first is not None:
            n_nan = int((np.isnan(results[first].estimate) & ~own).sum())
            if n_nan:
                logger.warning(f"jackknife: {n_nan} entries of {first} are NaN (a channel without power in a bin)")
        first = next((k for k in names if k in _lib.JACKKNIFE_PHASE_MEASURES), None)
        if first is not None:
            nan = np.isnan(results[first].estimate) & ~own
            if first == "debiased_squared_weighted_phase_lag_index" and self._device().real_input:
                nan[..., 0, :, :] = False                            # (Im s = 0 in every observation of the zero and Nyquist bins
                if self._shape5[3] % 2 == 0:                         # of a real series: NaN by the measure's definition)
                    nan[..., -1, :, :] = False
            if nan.any():
                logger.warning(f"jackknife: {int(nan.sum())} entries of {first} are NaN (coefficients that are not finite, or a pair "
                               "whose sum |Im s|^2 equals its sum (Im s)^2)")
        return SeedJackknife(results, seeds, all_targets)

    def _seed_jackknife_sums(self, seeds, targets, mask, planes, over_id, n_units):
        """(the library's output as a flat float64 NumPy array: theta, sum d, sum d^2 per measure of the mask; n_bins).  The spectra
        are those ``seed_connectivity`` reads (_seed_spectra: no planes hint, the amplitude guard for requests that read (Im s)^2).
        The total is a seed record of doubles that the jackknife sums from these spectra itself (_stage_d.seed_jackknife_totals),
        summed over every rank's trials and cached; a later request with the same seeds, targets, ``over`` and spectra that needs
        no other plane reads it again."""
        from . import _stage_d
        sp = self._seed_spectra(planes & ~_lib.SEED_PLANE_POWER, "seed_jackknife")
        mem = self._memory(sp.X)
        who = (seeds.tobytes(), None if targets is None else targets.tobytes(), over_id, bool(sp.f64))
        mine = [k for k in self._accum_cache if isinstance(k, tuple) and k[0] == "seed_jackknife" and k[2:] == who]
        have = next((k for k in mine if k[1] & planes == planes), None)
        if have is None:
            total = _stage_d.seed_jackknife_totals(mem, sp, self.expectation_type, seeds, targets, planes, over_id, n_freq=self._n_freq)
            for old in [k for k in mine if k[1] & planes == k[1]]:
                del self._accum_cache[old]             # a record the new one covers: its memory can go
            have = ("seed_jackknife", planes) + who
            self._accum_cache[have] = (self._reduce_over_ranks(total), None)
        out, n_bins = _stage_d.seed_jackknife(mem, sp, self.expectation_type, seeds, targets, self._accum_cache[have][0], have[1], mask,
                                              over_id, n_units, n_freq=self._n_freq)
        n_targets = int(self._shape5[4]) if targets is None else len(targets)
        return mem.download(self._seed_jackknife_reduce(out, n_bins * len(seeds) * n_targets)), n_bins

    def _seed_jackknife_reduce(self, out, size):
        """Sum of the partial sums over the processes that hold the trials (nothing to add here).  ``size``: doubles of one of the
        three arrays -- theta, sum d, sum d^2 -- of every measure in ``out``."""
        return out

    def conditional_spectral_granger_prediction(self):
        """Power at node i explained by node j given every other signal, out[..., i, j] = j -> i | rest (diagonal NaN;
        Geweke 1984, Ding, Chen & Bressler 2006 section 3.3 -- the reference raises NotImplementedError,
        connectivity.py:1215-1224).  The full factor is the cached one of the MVAR measures; one reduced Wilson
        factorisation per dropped signal runs on the device (sc_conditional.hip).  With two signals this is the pairwise
        measure.  ``_last_wilson`` then describes the reduced factorisations (n_iter / status [n_signals, n_groups])."""
        from . import _stage_d
        N, C = self._shape5[3], self._shape5[4]
        self._check_mvar_signals()
        G = self._mvar_factor_device()
        accum, n_obs, n_freq = self._csm_records("granger")
        mem = self._memory(accum)
        out, n_iter, status, summary = _stage_d.conditional_granger(
            mem, G, accum.shape[0] // n_freq, N, C, accum=accum, n_freq_accum=n_freq, planes=_lib.PLANE_CSM,
            n_obs=self._n_observations_total(n_obs))
        self._wilson_done(mem, "reduced problems", summary, n_iter, status)
        return mem.download(out).reshape(self._kept_shape() + (N // 2 + 1, C, C))

    # (the reference declares the method without arguments, tests/golden/api_surface.json: group_labels is bound here)
    def blockwise_spectral_granger_prediction(self, *args, **kwargs):
        """Power in group a explained by group b, out[..., a, b] = b -> a, for groups of signals (Geweke 1982, multivariate
        form -- the reference raises NotImplementedError, connectivity.py:1226-1235).  ``group_labels``: one label per signal;
        returns (values [kept axes..., n_freq, n_groups, n_groups] float64 with a NaN diagonal, np.unique(group_labels)).
        One Wilson factorisation of the n_a + n_b signals of every group pair runs on the device (sc_blockwise.hip), so a pair
        may have up to sc_mvar_max_signals() signals whatever the total.  A pair with more signals than observations has a
        rank-deficient spectrum and is NaN (one warning counts them).  ``_last_wilson`` then describes the pair factorisations
        (n_iter / status [computed pairs, n_groups], pairs in order of their size m, then of the labels)."""
        return self._blockwise_granger(*args, **kwargs)

    def _blockwise_pairs(self, group_labels):
        return _lib.blockwise_pairs(group_labels, self._shape5[4], int(_lib.load().sc_mvar_max_signals()))

    def _blockwise_batches(self, pairs, n_obs_total):
        batches, n_skipped = _lib.blockwise_batches(pairs, n_obs_total)
        if n_skipped:
            logger.warning(f"blockwise Granger: {n_skipped} group pairs have more signals than the {n_obs_total} observations "
                           "(rank-deficient spectra): NaN")
        return batches

    def _blockwise_granger(self, group_labels):
        from . import _stage_d
        N = self._shape5[3]
        labels, pairs = self._blockwise_pairs(group_labels)      # (the labels are checked before any device work)
        accum, n_obs, n_freq = self._csm_records("granger")
        n_total = self._n_observations_total(n_obs)
        batches = self._blockwise_batches(pairs, n_total)
        mem = self._memory(accum)
        out, n_iter, status, summary = _stage_d.blockwise_granger(
            mem, accum.shape[0] // n_freq, N, self._shape5[4], batches, len(labels), accum=accum, n_freq_accum=n_freq,
            planes=_lib.PLANE_CSM, n_obs=n_total)
        self._wilson_done(mem, "group-pair problems", summary, n_iter, status)
        return mem.download(out).reshape(self._kept_shape() + (N // 2 + 1, len(labels), len(labels))), labels
