"""``Multitaper`` / ``Connectivity`` on the torch-free host: the reference's own dependencies (NumPy + SciPy,
``pyproject.toml:42-47``) and ``libsc_hip.so`` -- nothing else.

``spectral_connectivity_amd.Connectivity`` sits on one of two hosts of the same C ABI (``include/sc_hip.h``):

* the PyTorch host (``engine.py``): torch owns the HBM buffers, the stream and the RCCL collectives of the multi-GPU path;
* this one (``numpy_host.NumpyHost``: ctypes + NumPy over the library's own allocator, copies and stream).

``SC_HIP_HOST=numpy|torch`` selects (default: torch when it can be imported, NumPy otherwise); with ``numpy`` the package's
``Connectivity`` is the class below and ``Multitaper.fft()`` / ``Multitaper.device_spectra()`` run here -- ``torch`` is never
imported.  Same constructor, properties, methods, shapes, dtypes, warnings and errors as the PyTorch-host class (it IS that class:
only the methods of stages A-C that touch the device are replaced, and they call the same drivers, ``_stage_abc.py``, through
``NumpyHost.memory``; stage D runs the base class's methods over the shared drivers of ``_stage_d.py`` the same way), both engines (``dtype=complex64`` -> float32 engine, planes format
included; ``complex128``, the default -> float64 engine), every expectation-type measure, pairwise / subset Granger, the full
Wilson factor and the directed MVAR measures, canonical and global coherence, MIC / MIM, the jackknife, the band statistics, more than 256
signals (channel blocks of 128, tiled on the host).  Not here: complex-valued time series, multi-GPU (``parallel.ShardedConnectivity`` needs
``torch.distributed``), hipGraph replay (``engine.GraphedMeasures``).
"""
import numpy as np

from . import _lib, _stage_abc, _stage_d
from .connectivity import Connectivity as _TorchHostConnectivity
from .connectivity import InteractionVectors, _PendingSpectra
from .numpy_host import DeviceArray as _Record      # accumulator records on the device: [n_bins][floats_per_bin] float32 / float64

_host = None


def host():
    """The process-wide NumpyHost (one HIP runtime per process: see _lib.load())."""
    global _host
    if _host is None:
        from .numpy_host import NumpyHost
        _host = NumpyHost()
    return _host


def multitaper_spectra(m, precision, planes_hint=None):
    """Multitaper.device_spectra of this host."""
    h = host()
    if np.iscomplexobj(m.time_series):
        raise TypeError("complex-valued time series need the PyTorch host (SC_HIP_HOST=torch): it transforms the real and imaginary "
                        "parts with the real-input kernels and assembles the two-sided spectrum on the device")
    ts = np.asarray(m.time_series)
    if ts.shape[2] > 256:
        # more than 256 signals: planes-format spectra of the whole array where the format applies (round 6: sc_fused2.hip plans its
        # launches over any number of 32-channel blocks) -- otherwise no device spectra of the whole array, the record is tiled
        C = ts.shape[2]
        C_alloc = _lib.padded_channels(C, _lib.PLANES_FORMAT_MAX_CHANNELS)
        F, W, R, K = m.n_fft_samples // 2 + 1, int(m.n_time_windows), ts.shape[1], int(m.n_tapers)
        if (precision != "float64" and C_alloc <= _lib.PLANES_FORMAT_MAX_CHANNELS
                and _lib.planes_format_applies(m.n_time_samples_per_window, m.n_fft_samples, C_alloc, planes_hint,
                                               spectra_bytes=F * W * R * K * C_alloc * 8)):
            sp = h.spectra(m, planes_hint=planes_hint)
            if sp.P is not None:
                sp.wide_source = (m, precision)       # (a family outside the format later: back to the tiling, see _accumulators)
                return sp
            sp.free()                                    # (the format's quality check sent the transform to complex64)
        return _WideSeries(m, precision)
    return h.spectra_f64(m) if precision == "float64" else h.spectra(m, planes_hint=planes_hint)


class _WideSeries:
    """More than 256 signals: no device spectra of the whole array (one launch of the stage-B kernels stages <= 256 channels) --
    the record is tiled from the spectra of channel-block pairs (Connectivity._accumulate_wide)."""
    is_device_spectra = True

    def __init__(self, multitaper, precision):
        self.multitaper, self.precision = multitaper, precision
        ts = np.asarray(multitaper.time_series)
        self.W, self.R, self.K = int(multitaper.n_time_windows), int(ts.shape[1]), int(multitaper.n_tapers)
        self.n_fft, self.C = int(multitaper.n_fft_samples), int(ts.shape[2])
        self.F = self.n_fft // 2 + 1
        self.real_input, self.f64, self.P = True, precision == "float64", None


def fft(m):
    """Multitaper.fft() of this host: (n_time_windows, n_trials, n_tapers, n_fft_samples, n_signals) complex128, two-sided."""
    from . import options
    precision = options.engine_precision(None)
    ts = np.asarray(m.time_series)
    C = ts.shape[2]
    cols = [np.arange(c0, min(c0 + 256, C)) for c0 in range(0, C, 256)]
    parts = []
    for cc in cols:
        sub = m if len(cols) == 1 else _channel_subset_multitaper(m, cc)
        sp = host().spectra_f64(sub) if precision == "float64" else host().spectra(sub)
        dt = np.complex128 if sp.f64 else np.complex64
        one = host().download(sp.X, (sp.F, sp.W, sp.R, sp.K, sp.C_alloc), dt)[..., :sp.C]
        parts.append(np.array(one, dtype=np.complex128))
        sp.free()
    one = np.moveaxis(parts[0] if len(parts) == 1 else np.concatenate(parts, axis=-1), 0, 3)       # (W, R, K, F, C)
    N, F = m.n_fft_samples, one.shape[3]
    out = np.empty(one.shape[:3] + (N, one.shape[-1]), dtype=np.complex128)
    out[..., :F, :] = one
    if N > F:
        out[..., F:, :] = np.conj(one[..., N - F:0:-1, :])
    return out


def _channel_subset_multitaper(m, cols):
    """The same transform for the channels ``cols`` of the series (stage A is per channel: nothing else changes): a shallow copy of
    the object -- every resolved parameter, the tapers -- with the series replaced."""
    import copy
    _ = m.tapers                                           # (resolved once, shared by the copies)
    sub = copy.copy(m)
    sub.time_series = np.ascontiguousarray(np.asarray(m.time_series)[:, :, cols])
    sub._device_spectra, sub._deferred_checks = None, None
    sub._finite_checked = True                             # (the constructor's scan was the whole series')
    return sub


class Connectivity(_TorchHostConnectivity):
    """``spectral_connectivity_amd.Connectivity`` on the torch-free host (module docstring)."""

    @classmethod
    def from_multitaper(cls, multitaper_instance, expectation_type="trials_tapers", blocks=None, dtype=np.complex128):
        """Reference connectivity.py:366-400; the transform runs at the first request (its accumulator families decide the device
        format of the float32 engine's spectra)."""
        from . import options
        precision = options.engine_precision(dtype)
        multitaper_instance.check_device_path()
        if np.iscomplexobj(multitaper_instance.time_series):
            raise TypeError("complex-valued time series need the PyTorch host (SC_HIP_HOST=torch)")
        obj = cls(_PendingSpectra(multitaper_instance, precision), expectation_type=expectation_type,
                  time=multitaper_instance.time, frequencies=multitaper_instance.frequencies, blocks=blocks, dtype=dtype)
        obj._multitaper = multitaper_instance
        return obj

    # ---- device plumbing -----------------------------------------------------------------------------------------------------
    def _device(self, planes_hint=None, defer_checks=False):
        if self._spectra is None and self._pending is not None:
            if planes_hint is not None and not (planes_hint in _lib.PLANES_FORMAT_FAMILIES and self._planes_request_ok(planes_hint)):
                planes_hint = None
            self._spectra = multitaper_spectra(self._pending.multitaper, self._pending.precision, planes_hint)
            self._pending = None
        if self._spectra is None:
            _lib.require_gpu()
            if self._host_coefficients.shape[-1] > 256:
                raise ValueError("uploaded coefficients of more than 256 signals: build the object with Connectivity.from_multitaper "
                                 "(the channel blocks are transformed from the series) or use the PyTorch host")
            self._spectra = host().upload_coefficients(self._host_coefficients, f64=self._precision == "float64")
        return self._spectra

    def _settle(self):
        return True

    def _accumulate(self, sp, expectation_type, planes, n_freq):
        if isinstance(sp, _WideSeries):
            return self._accumulate_wide(sp, expectation_type, planes, n_freq)
        return host()._accumulate_record(sp, expectation_type, planes, n_freq)

    def _accumulate_wide(self, wide, expectation_type, planes, n_freq):
        """engine._accumulate_blocked on this host: every pair of channel blocks (_lib.tile_plan) is a request of its own (<= 256
        signals: the ordinary kernels, spectra of just those channels from the series), its 16 x 16 record tiles are placed into the
        full record on the HOST, and the full record goes back to the device once for whatever consumes it."""
        m = wide.multitaper
        NB = -(-wide.C // 16)
        full, n_obs_out = None, None
        for _, _, cols, src, dst in _lib.tile_plan(wide.C):
            sub_m = _channel_subset_multitaper(m, cols)
            sp = host().spectra_f64(sub_m) if wide.f64 else host().spectra(sub_m)
            part, n_obs = host()._accumulate_record(sp, expectation_type, planes, n_freq)
            sp.free()
            nb_s = -(-len(cols) // 16)
            nt_s = nb_s * (nb_s + 1) // 2
            n_bins = part.shape[0]
            dt = np.dtype(part.dtype)      # (float32 engine: float64 for a block pair outside the float32 range, _stage_abc.amplitude_guard)
            rec = np.array(host().download(part.buf, (n_bins, part.shape[1] // (nt_s * 256), nt_s, 256), dt))
            del part
            if full is None:
                full, n_obs_out = np.zeros((n_bins, rec.shape[1], NB * (NB + 1) // 2, 256), dtype=dt), n_obs
            elif dt.itemsize > full.dtype.itemsize:
                full = full.astype(dt)
            full[:, :, dst] = rec[:, :, src]
        full = full.reshape(full.shape[0], -1)
        return _Record(host().upload(full), full.shape, full.dtype), n_obs_out

    def _accumulators(self, planes, defer_checks=False):
        for have, rec in self._accum_cache.items():
            if isinstance(have, int) and have & planes == planes:
                return have, rec
        from . import options
        sp = self._device(planes_hint=planes)
        if (getattr(sp, "P", None) is not None and planes == _lib.PLANE_CSM and options.anticipate_phase_lag
                and self._planes_request_ok(_lib.PLANE_CSM | _lib.PLANE_ABS_IM)):
            planes = _lib.PLANE_CSM | _lib.PLANE_ABS_IM            # (Connectivity._accumulators: coherence then wPLI is one pass)
        elif getattr(sp, "f64", False) and planes == _lib.PLANE_CSM and options.anticipate_phase_lag and not isinstance(sp, _WideSeries):
            # float64 engine on this host: a later phase-lag request cannot copy the families a record already holds (the PyTorch
            # host does, with a strided device copy) and would accumulate everything again -- the |Im s| plane rides along instead
            planes = _lib.PLANE_CSM | _lib.PLANE_ABS_IM
        if getattr(sp, "P", None) is not None and not _stage_abc.fused2_takes(sp.desc(self.expectation_type, self._n_freq, padded=True),
                                                                             planes):
            # spectra held as f16 pieces, and a family their kernels do not take (PLV after coherence, ...): decoded once
            self._spectra = sp = self._decode_planes(sp)
        rec, n_obs = self._accumulate(sp, self.expectation_type, planes, self._n_freq)
        for old in [h for h in self._accum_cache if isinstance(h, int) and h & planes == h]:
            del self._accum_cache[old]
        self._accum_cache[planes] = (rec, n_obs)
        return planes, (rec, n_obs)

    def _decode_planes(self, sp):
        """complex64 spectra from the planes format (sc_spectra_from_planes_f32: lossless up to its 22 bits).  More than 256 signals:
        the complex64 kernels do not take them in one piece -- back to the series and the channel-block tiling."""
        if sp.C > 256:
            m, precision = sp.wide_source
            sp.free()
            return _WideSeries(m, precision)
        mem = host().memory
        out = mem.spectra(_stage_abc.decode_planes(mem, sp), (sp.F, sp.W, sp.R, sp.K, sp.C), sp.strides, sp.n_fft, sp.real_input,
                          C_alloc=sp.C_alloc)
        sp.free()
        return out

    def _csm_records(self, tag, expectation_type=None, two_sided=True):
        sp = self._device()
        if getattr(sp, "P", None) is not None:
            self._spectra = sp = self._decode_planes(sp)
        N = self._shape5[3]
        n_freq = (sp.F if sp.real_input else N) if two_sided else self._n_freq
        key = (tag, n_freq)
        if key not in self._accum_cache:
            self._accum_cache[key] = self._accumulate(sp, expectation_type or self.expectation_type, _lib.PLANE_CSM, n_freq)
        rec, n_obs = self._accum_cache[key]
        return rec, n_obs, n_freq

    @property
    def _shape5(self):
        if self._host_coefficients is not None:
            return self._host_coefficients.shape
        if self._spectra is None and self._pending is not None:
            return self._pending.shape5
        s = self._spectra
        return (s.W, s.R, s.K, s.n_fft, s.C)

    # ---- stage C --------------------------------------------------------------------------------------------------------------
    def _measure(self, which):
        have, (rec, n_obs) = self._accumulators(_lib.MEASURE_PLANES[which])
        C = self._shape5[4]
        out = _stage_abc.measure(host().memory, rec, C, have, self._n_observations_total(n_obs), which, self._wide_output(which))
        res = host().download(out.buf, out.shape, out.dtype)        # (the page-locked array itself: its owner recycles the block with the last view)
        del out
        tail = (C,) if which == _lib.M_POWER else (C, C)
        return res.reshape(self._kept_shape() + (self._n_freq,) + tail)

    # ---- stage D: the base class's methods run the shared drivers (_stage_d.py) through this host's memory adapter; what is left
    # here places the downloaded results where the base class works on device tensors (for parallel.ShardedConnectivity) ----------
    def _memory(self, like=None):
        return host().memory

    def canonical_coherence(self, group_labels):
        rec, n_obs, _ = self._csm_records("canonical", "trials_tapers", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        labels, groups, small = self._canonical_groups(group_labels, n_total)
        n_g, n_bins = len(groups), rec.shape[0]
        res = np.ones((n_bins, n_g, n_g))
        res[:, np.arange(n_g), np.arange(n_g)] = np.nan
        if len(small) >= 2:
            mem = self._memory()
            sub, n_fail = _stage_d.canonical_coherence(mem, rec, self._shape5[4], _lib.PLANE_CSM, n_total, [groups[k] for k in small])
            res[np.ix_(np.arange(n_bins), small, small)] = mem.download(sub)
            self._canonical_failed(n_fail)
        return res.reshape(self._shape5[0], self._n_freq, n_g, n_g), labels

    def canonical_coherence_vectors(self, group_labels):
        group_labels = self._canonical_labels(group_labels)                     # (the labels are checked before any device work)
        rec, n_obs, _ = self._csm_records("canonical", "trials_tapers", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        labels, groups, small = self._canonical_groups(group_labels, n_total)
        G, n_bins, n_max = len(groups), rec.shape[0], max(len(g) for g in groups)
        coherence = np.ones((n_bins, G, G))
        coherence[:, np.arange(G), np.arange(G)] = np.nan
        coherences = np.broadcast_to(self._canonical_ones(groups), (n_bins, G, G, n_max)).copy()
        filters, patterns = np.full((n_bins, G, G, n_max, 2), np.nan), np.full((n_bins, G, G, n_max, 2), np.nan)
        if len(small) >= 2:
            mem = self._memory()
            sub_members, sub_sizes, _ = _lib.member_table([groups[k] for k in small])
            c, cs, f, p, n_fail = _stage_d.canonical_coherence_vectors(mem, rec, self._shape5[4], _lib.PLANE_CSM, n_total, sub_members,
                                                                       sub_sizes)
            n_sub = int(sub_sizes.max())
            cells = np.ix_(np.arange(n_bins), small, small)
            coherence[cells] = mem.download(c)
            coherences[cells] = np.nan
            cells = np.ix_(np.arange(n_bins), small, small, np.arange(n_sub))
            coherences[cells] = mem.download(cs)
            filters[cells], patterns[cells] = mem.download(f), mem.download(p)
            self._canonical_failed(n_fail)
        return self._canonical_vectors_result((coherence, coherences, filters, patterns), labels, groups)

    canonical_coherence_vectors.__doc__ = _TorchHostConnectivity.canonical_coherence_vectors.__doc__

    def _jackknife_sums(self, mask, over_id, n_units):
        if self._shape5[4] > 256:
            # (this host holds no complex spectra of more than 256 signals: _WideSeries, _decode_planes)
            raise ValueError("jackknife of more than 256 signals needs device spectra of the whole array: use the PyTorch host "
                             "(SC_HIP_HOST=torch)")
        return super()._jackknife_sums(mask, over_id, n_units)

    def _jackknife_phase_sums(self, mask, planes, over_id, n_units):
        if self._shape5[4] > 256:
            raise ValueError("jackknife of more than 256 signals needs device spectra of the whole array: use the PyTorch host "
                             "(SC_HIP_HOST=torch)")
        sp = self._device()
        if getattr(sp, "P", None) is not None:          # (the kernel reads complex64: spectra held as f16 pieces are decoded once)
            self._spectra = self._decode_planes(sp)
        return super()._jackknife_phase_sums(mask, planes, over_id, n_units)

    def _seed_spectra(self, planes, method="seed_connectivity"):
        if self._shape5[4] > 256:
            raise ValueError(f"{method} of more than 256 signals needs device spectra of the whole array: use the PyTorch host "
                             "(SC_HIP_HOST=torch)")
        sp = self._device()
        if getattr(sp, "P", None) is not None:          # (the kernel reads complex64: spectra held as f16 pieces are decoded once)
            self._spectra = sp = self._decode_planes(sp)
        return _stage_abc.amplitude_guard(host().memory, sp, planes)

    def _imaginary_interaction(self, group_labels):
        labels, members, sizes, _ = self._interaction_groups(group_labels)      # (the labels are checked before any device work)
        rec, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        keep = self._interaction_kept(sizes, n_total)
        G, n_bins = len(labels), rec.shape[0]
        mic, mim = np.full((n_bins, G, G), np.nan), np.full((n_bins, G, G), np.nan)
        if len(keep) >= 2:
            mem = self._memory()
            sub_members, sub_sizes, _ = _lib.member_table([members[k, :sizes[k]] for k in keep])
            a, b, n_fail = _stage_d.imaginary_interaction(mem, rec, self._shape5[4], _lib.PLANE_CSM, n_total, sub_members, sub_sizes)
            cells = np.ix_(np.arange(n_bins), keep, keep)
            mic[cells], mim[cells] = mem.download(a), mem.download(b)
            self._interaction_failed(n_fail)
        shape = self._kept_shape() + (self._n_freq, G, G)
        return mic.reshape(shape), mim.reshape(shape), labels

    def maximized_imaginary_coherence_vectors(self, group_labels):
        labels, members, sizes, _ = self._interaction_groups(group_labels)      # (the labels are checked before any device work)
        rec, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        keep = self._interaction_kept(sizes, n_total)
        G, n_bins, n_max = len(labels), rec.shape[0], int(sizes.max())
        mic = np.full((n_bins, G, G), np.nan)
        filters, patterns = np.full((n_bins, G, G, n_max), np.nan), np.full((n_bins, G, G, n_max), np.nan)
        if len(keep) >= 2:
            mem = self._memory()
            sub_members, sub_sizes, _ = _lib.member_table([members[k, :sizes[k]] for k in keep])
            a, f, p, n_fail = _stage_d.imaginary_interaction_vectors(mem, rec, self._shape5[4], _lib.PLANE_CSM, n_total, sub_members,
                                                                     sub_sizes)
            n_sub = int(sub_sizes.max())
            mic[np.ix_(np.arange(n_bins), keep, keep)] = mem.download(a)
            cells = np.ix_(np.arange(n_bins), keep, keep, np.arange(n_sub))
            filters[cells], patterns[cells] = mem.download(f), mem.download(p)
            self._interaction_failed(n_fail)
        shape = self._kept_shape() + (self._n_freq, G, G)
        return InteractionVectors(mic.reshape(shape), filters.reshape(shape + (n_max,)), patterns.reshape(shape + (n_max,)), labels,
                                  [members[g, :sizes[g]].astype(np.int64) for g in range(G)])

    maximized_imaginary_coherence_vectors.__doc__ = _TorchHostConnectivity.maximized_imaginary_coherence_vectors.__doc__

    def _linear_dependence(self, group_labels, want):
        labels, members, sizes, _ = self._dependence_groups(group_labels)       # (the labels are checked before any device work)
        rec, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        mem = self._memory()
        res, n_fail = _stage_d.linear_dependence(mem, rec, self._shape5[4], _lib.PLANE_CSM, n_total, members, sizes, want)
        self._dependence_warnings(sizes, n_total, n_fail)
        shape = self._kept_shape() + (self._n_freq, len(labels), len(labels))
        return {name: np.array(mem.download(res[name])).reshape(shape) for name in want}, labels

    def _partial_coherence(self, name):
        C, _, shape, dtype = self._partial_shape(name)
        rec, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        if self._partial_few_observations(n_total, C):
            return np.full(shape, np.nan, dtype=dtype)
        mem = self._memory()
        res, n_fail = _stage_d.partial_coherence(mem, rec, C, _lib.PLANE_CSM, n_total, (name,))
        self._partial_failed(n_fail)
        return mem.download(res[name]).reshape(shape)

    def _partial_coherence_given(self, name, given, signals):
        kept, z, _, shape, dtype = self._partial_given_request(name, given, signals)
        rec, n_obs, _ = self._csm_records("interaction", two_sided=False)
        n_total = self._n_observations_total(n_obs)
        if self._partial_given_few_observations(n_total, len(z)):
            return np.full(shape, np.nan, dtype=dtype)
        mem = self._memory()
        res, counts = _stage_d.partial_coherence_given(mem, rec, self._shape5[4], _lib.PLANE_CSM, n_total, kept, z, (name,))
        self._partial_given_failed(counts)
        return mem.download(res[name]).reshape(shape)
