"""The thin host BASELINE.json's north_star names: ctypes + NumPy over the C ABI of ``include/sc_hip.h`` -- no torch.

``spectral_connectivity_amd.Connectivity`` sits on a PyTorch host (torch owns HBM buffers, streams and the RCCL
collectives of the multi-GPU path).  This module drives the SAME library with nothing but NumPy arrays: device and
page-locked memory, copies and the stream come from the library's own ``sc_device_alloc`` / ``sc_host_alloc`` /
``sc_memcpy_*`` / ``sc_stream_*`` entry points (sc_memory.hip), the way the reference's CuPy backend uploads with
``xp.asarray`` and downloads with ``.get()`` (reference transforms.py:405-439, connectivity.py:31-65).

    from spectral_connectivity_amd.numpy_host import NumpyHost
    host = NumpyHost()
    out = host.connectivity(time_series, sampling_frequency=1000, time_halfbandwidth_product=4,
                            n_time_samples_per_window=256, n_time_samples_per_step=128,
                            measures=("coherence_magnitude", "weighted_phase_lag_index"))

The call sequences are the PyTorch host's: the shared drivers of ``_stage_abc.py`` (stages A to C) and ``_stage_d.py`` run here
through ``NumpyMemory``; what this module adds is the memory (``DeviceBuffer`` / ``DeviceArray`` / ``PinnedArray``), the spectra
object ``NpSpectra`` and this host's policy -- the planes format's quality check is read at once, an FFT plan lives for one transform.

Scope of the functional interface below: the float32 engine's hot path -- stage A (fused transform, or tapered windows + rocFFT
for the lengths the fused kernel does not take), stage B (every accumulator plane), the expectation-type measures of the reference
(connectivity.py:612-1159), ``expectation_type`` as in the reference -- and stage D on float32 records:
``pairwise_spectral_granger_prediction``, ``canonical_coherence``, ``mvar_measures`` (the full Wilson factor) and
``global_coherence``.  Results are float64 / complex128 NumPy arrays shaped like the reference's.  The float64 engine, the
other stage-D measures and more than 256 signals are on this host too, through the public classes (``numpy_api``, SC_HIP_HOST=numpy);
multi-GPU needs the PyTorch host.  One process uses one host: see _lib.load().
"""
import contextlib
import ctypes
from ctypes import byref, c_void_p

import numpy as np

from . import _lib, _stage_abc, _stage_d

EXPECTATION_AXES = _lib.EXPECTATION_AXES
MEASURES = {
    "power": _lib.M_POWER, "coherency": _lib.M_COHERENCY, "coherence_magnitude": _lib.M_COHERENCE_MAGNITUDE,
    "coherence_phase": _lib.M_COHERENCE_PHASE, "imaginary_coherence": _lib.M_IMAGINARY_COHERENCE,
    "phase_locking_value": _lib.M_PLV, "phase_lag_index": _lib.M_PLI, "weighted_phase_lag_index": _lib.M_WPLI,
    "debiased_squared_phase_lag_index": _lib.M_DEBIASED_PLI2,
    "debiased_squared_weighted_phase_lag_index": _lib.M_DEBIASED_WPLI2, "pairwise_phase_consistency": _lib.M_PPC,
}


class DeviceBuffer:
    """``n_bytes`` of HBM.  Blocks come from the library's stream-ordered pool ONCE and are then recycled by this host: a
    dropped buffer waits in ``host._released`` until the host has synchronised its stream, and only then serves the next
    request of its size class.  (Handing blocks back to the driver's pool with hipFreeAsync and taking them out again in
    stream order -- legal, and what this class did first -- gave intermittently corrupted measure buffers under
    /opt/rocm 7.2's runtime as soon as a large block was carved up differently from call to call (planes-format spectra
    where the previous call's output lay); the same sequence on the runtime PyTorch ships ran clean.  Recycling whole blocks
    at synchronisation points does not depend on either.)"""

    def __init__(self, host, n_bytes):
        self._host, self.n_bytes = host, int(n_bytes)
        self._size_class = DeviceBuffer.size_class(self.n_bytes)
        free = host._free_blocks.get(self._size_class)
        if free:
            self.ptr = c_void_p(free.pop())
            return
        p = c_void_p()
        _lib.check(host.lib.sc_device_alloc(byref(p), self._size_class, host.stream), "sc_device_alloc")
        self.ptr = p

    @staticmethod
    def size_class(n_bytes):
        """Request rounded up to 512 bytes below 1 MB and to 1/16 of its power of two above (<= 6 % of slack)."""
        n = max(int(n_bytes), 1)
        if n <= (1 << 20):
            return -(-n // 512) * 512
        step = 1 << (n.bit_length() - 5)
        return -(-n // step) * step

    def free(self):
        if self.ptr is not None and self.ptr.value:
            self._host._released.append((self._size_class, self.ptr.value))     # reusable after the next synchronize()
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceArray:
    """A DeviceBuffer that knows its shape and dtype: what this host holds where the PyTorch host holds a tensor (accumulator
    records [n_bins][floats_per_bin], the arrays of the stage-D drivers).  The memory goes back with the buffer."""

    def __init__(self, buf, shape, dtype):
        self.buf, self.shape, self.dtype = buf, tuple(int(n) for n in shape), np.dtype(dtype)

    @property
    def f64(self):
        return self.dtype == np.float64


class NumpyMemory:
    """The memory adapter of the shared drivers (_stage_abc.py, _stage_d.py) on this host: DeviceArray over NumpyHost.alloc / upload /
    download."""

    def __init__(self, host):
        self.host = host

    def empty(self, shape, dtype):
        dtype = np.dtype(dtype)
        return DeviceArray(self.host.alloc(int(np.prod(shape, dtype=np.int64)) * dtype.itemsize), shape, dtype)

    def zeros(self, shape, dtype):
        a = self.empty(shape, dtype)
        if a.buf.n_bytes:
            _lib.check(self.host.lib.sc_memset_zero(a.buf.ptr, a.buf.n_bytes, self.host.stream), "sc_memset_zero")
        return a

    def upload(self, array):
        array = np.ascontiguousarray(array)
        return DeviceArray(self.host.upload(array), array.shape, array.dtype)

    def ptr(self, a, first_row=0):
        """(``a``: a DeviceArray, or the raw DeviceBuffer of the spectra)"""
        if not first_row:
            return getattr(a, "buf", a).ptr
        return c_void_p(a.buf.ptr.value + first_row * int(np.prod(a.shape[1:], dtype=np.int64)) * a.dtype.itemsize)

    def stream(self):
        return self.host.stream

    def is_f64(self, record):
        return record.f64

    def read_scales(self, spectra):
        return np.array(self.host.download(spectra.scale, (2 * spectra.C_alloc,), np.float32))

    def fill_nan(self, a):
        src = np.full(a.shape, np.nan, dtype=a.dtype)
        _lib.check(self.host.lib.sc_memcpy_h2d(a.buf.ptr, src.ctypes.data_as(c_void_p), src.nbytes, self.host.stream), "sc_memcpy_h2d")
        self.host.synchronize()

    def read_int(self, a):
        return int(self.download(a).ravel()[0])

    def hstack(self, chunks, n_rows):
        if len(chunks) == 1:
            return chunks[0]
        return self.upload(np.concatenate([self.download(c).reshape(n_rows, -1) for c in chunks], axis=1).reshape(-1))

    def head(self, a, n):
        return DeviceArray(a.buf, (n,) + a.shape[1:], a.dtype)

    def spectra(self, X, dims, strides, n_fft, real_input, C_alloc=None, P=None, scale=None):
        X, f64 = (None, False) if X is None else (X.buf, X.dtype == np.complex128)
        return NpSpectra(X, dims, strides, n_fft, real_input, C_alloc, P and P.buf, scale and scale.buf, f64=f64)

    def twiddles(self, n_fft):
        tw = self.host._twiddles.get(n_fft)
        if tw is None:
            tw = self.host._twiddles[n_fft] = _stage_abc.make_twiddles(self, n_fft)
        return tw

    def workspace(self, n_bytes, owner=None):              # (a buffer of the call's own: back to the pool when the driver drops it)
        return self.empty((n_bytes,), np.uint8) if n_bytes > 0 else None

    @contextlib.contextmanager
    def fft_plan(self, n_fft, batch, f64=False):
        """A rocFFT plan for one execution: created, waited for, destroyed (its scratch must outlive the transform)."""
        lib, plan = self.host.lib, c_void_p()
        create = lib.sc_fft_plan_create_f64 if f64 else lib.sc_fft_plan_create
        _lib.check(create(byref(plan), n_fft, batch), "sc_fft_plan_create")
        try:
            yield plan
            self.host.synchronize()
        finally:
            lib.sc_fft_plan_destroy(plan)

    def download(self, a):
        """A NumPy array of its own (not the page-locked block, which goes back to the pool)."""
        if not a.buf.n_bytes:
            return np.zeros(a.shape, dtype=a.dtype)
        return np.array(self.host.download(a.buf, a.shape, a.dtype))


class PinnedArray(np.ndarray):
    """A NumPy array over page-locked memory of sc_host_alloc.  Page-locking is the expensive part (20 ms per 100 MB
    on the MI355X host, 12 ms to release), so the block goes back to a small pool with the last view of the array and
    the next result of that size reuses it: a steady-state download costs the copy alone (57 GB/s)."""

    _pool = {}                      # n_bytes -> [address, ...] of released blocks
    _pooled_bytes = 0
    POOL_LIMIT = 4 << 30

    @classmethod
    def empty(cls, lib, shape, dtype):
        dtype = np.dtype(dtype)
        n_bytes = max(int(np.prod(shape, dtype=np.int64)) * dtype.itemsize, 1)
        free = cls._pool.get(n_bytes)
        if free:
            address = free.pop()
            cls._pooled_bytes -= n_bytes
        else:
            p = c_void_p()
            _lib.check(lib.sc_host_alloc(byref(p), n_bytes), "sc_host_alloc")
            address = p.value
        raw = (ctypes.c_char * n_bytes).from_address(address)
        arr = np.frombuffer(raw, dtype=dtype, count=n_bytes // dtype.itemsize).reshape(shape).view(cls)
        arr._owner = _PinnedOwner(lib, address, n_bytes)
        return arr

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)

    @classmethod
    def trim(cls, lib):
        """Release the pooled blocks."""
        for blocks in cls._pool.values():
            for address in blocks:
                lib.sc_host_free(c_void_p(address))
        cls._pool.clear()
        cls._pooled_bytes = 0


class _PinnedOwner:
    def __init__(self, lib, address, n_bytes):
        self.lib, self.address, self.n_bytes = lib, address, n_bytes

    def __del__(self):
        try:
            if PinnedArray._pooled_bytes + self.n_bytes <= PinnedArray.POOL_LIMIT:
                PinnedArray._pool.setdefault(self.n_bytes, []).append(self.address)
                PinnedArray._pooled_bytes += self.n_bytes
            else:
                self.lib.sc_host_free(c_void_p(self.address))
        except Exception:
            pass


class NpSpectra(_stage_abc.Spectra):
    """Device spectra of this host (geometry and ``desc``: _stage_abc.Spectra): X / P / scale are DeviceBuffers or None, the
    ``quality`` scalar of the planes format a DeviceArray."""

    def get(self, name, default=None):                      # (sp.get("P"), sp["P"]: the mapping access of the dict this class was)
        return getattr(self, name, default)

    def __getitem__(self, name):
        return getattr(self, name)

    def free(self):
        for buf in (self._X, self.P, self.scale):
            if buf is not None:
                buf.free()
        self._X = self.P = self.scale = None


class NumpyHost:
    """One stream on the current device, buffers from the library, NumPy in and out."""

    def __init__(self):
        self.lib = _lib.load(torch_host=False)
        if _lib.gpu_switch() is False:
            raise RuntimeError(f"{_lib.ENABLE_GPU_ENV} selects the reference's NumPy backend, which this package does "
                               "not have: every computation runs on the HIP engine.")
        if _lib.device_count() < 1:
            raise RuntimeError("spectral_connectivity_amd: no ROCm GPU is visible. This engine has no CPU fallback; "
                               "run on an MI355X host.")
        s = c_void_p()
        _lib.check(self.lib.sc_stream_create(byref(s)), "sc_stream_create")
        self.stream = s
        self._twiddles = {}
        self._free_blocks, self._released = {}, []      # DeviceBuffer's block cache: size class -> [address], and the not-yet-safe ones
        self.memory = NumpyMemory(self)

    def close(self):
        if self.stream is not None:
            self._twiddles.clear()
            self.trim()
            PinnedArray.trim(self.lib)
            self.lib.sc_stream_destroy(self.stream)
            self.stream = None

    def synchronize(self):
        _lib.check(self.lib.sc_stream_synchronize(self.stream), "sc_stream_synchronize")
        # nothing queued can touch the buffers dropped so far any more: they may serve new requests
        released, self._released = self._released, []
        for size_class, address in released:
            self._free_blocks.setdefault(size_class, []).append(address)
        if sum(k * len(v) for k, v in self._free_blocks.items()) > self.CACHE_LIMIT:
            self.trim()                                  # (many different shapes through one host: start over)

    CACHE_LIMIT = 64 << 30

    def trim(self):
        """Hand the cached device blocks back to the library's pool."""
        _lib.check(self.lib.sc_stream_synchronize(self.stream), "sc_stream_synchronize")
        for size_class, address in self._released:
            self._free_blocks.setdefault(size_class, []).append(address)
        self._released = []
        for blocks in self._free_blocks.values():
            for address in blocks:
                self.lib.sc_device_free(c_void_p(address), self.stream)
        self._free_blocks.clear()

    # ---- memory -------------------------------------------------------------------------------------------------
    def alloc(self, n_bytes):
        return DeviceBuffer(self, n_bytes)

    def upload(self, array):
        """Contiguous NumPy array -> device buffer (asynchronous when the array is page-locked)."""
        pinned = isinstance(array, PinnedArray) and array.flags.c_contiguous     # (ascontiguousarray returns a base-class array)
        a = np.ascontiguousarray(array)
        buf = self.alloc(a.nbytes)
        _lib.check(self.lib.sc_memcpy_h2d(buf.ptr, a.ctypes.data_as(c_void_p), a.nbytes, self.stream), "sc_memcpy_h2d")
        if not pinned:
            self.synchronize()             # a pageable source may be reused by the caller as soon as this returns
        return buf

    def download(self, buf, shape, dtype):
        """Device buffer -> NumPy array in page-locked memory (the copy runs at link rate)."""
        out = PinnedArray.empty(self.lib, shape, dtype)
        _lib.check(self.lib.sc_memcpy_d2h(out.ctypes.data_as(c_void_p), buf.ptr, out.nbytes, self.stream), "sc_memcpy_d2h")
        self.synchronize()
        return out

    def has_nonfinite(self, buf, n, f64=False):
        """The constructor's NaN / infinity scan (reference transforms.py:746-753) on the uploaded series."""
        flag = self.alloc(4)
        _lib.check(self.lib.sc_memset_zero(flag.ptr, 4, self.stream), "sc_memset_zero")
        fn = self.lib.sc_nonfinite_f64 if f64 else self.lib.sc_nonfinite_f32
        _lib.check(fn(buf.ptr, n, flag.ptr, self.stream), "sc_nonfinite")
        return bool(self.download(flag, (1,), np.int32)[0])

    # ---- stages A to C: the shared drivers of _stage_abc.py through self.memory; what stays here is this host's policy ----------
    def _series_checks(self, m, what):
        if np.iscomplexobj(m.time_series):
            raise TypeError(what)
        _stage_abc.check_detrend(m.detrend_type)

    def _warn_nonfinite(self, m, x, f64=False):
        """The constructor's deferred NaN / infinity scan on the uploaded (float32 engine: converted and padded) series."""
        if getattr(m, "_finite_checked", True) is False and self.has_nonfinite(x.buf, int(np.prod(x.shape)), f64=f64):
            import warnings
            warnings.warn(_stage_abc.NONFINITE_WARNING, UserWarning, stacklevel=4)

    def spectra(self, multitaper, planes_hint=None):
        """Stage A for a ``transforms.Multitaper`` (host geometry, tapers): NpSpectra with the device spectra
        X[F][W][R][K][C_alloc] complex64 -- or, when the accumulator families ``planes_hint`` the caller will
        ask for take it (``_lib.planes_format_applies``), the same coefficients in the planes format of sc_fused2.hip:
        P (rows of sc_planes_row_bytes) + the per-channel scales, X = None."""
        m, mem = multitaper, self.memory
        self._series_checks(m, "complex-valued time series: use the PyTorch host (spectral_connectivity_amd.Multitaper), which "
                               "transforms the real and imaginary parts and assembles the two-sided spectrum")
        ts = np.asarray(m.time_series)
        T, R, C = ts.shape
        C_alloc = _lib.padded_channels(C, _lib.PLANES_FORMAT_MAX_CHANNELS)       # (beyond 256 signals: planes-format requests only)
        h32 = np.ascontiguousarray(np.asarray(m.tapers, dtype=np.float64).T / m.sampling_frequency, dtype=np.float32)   # (K, L)
        h = mem.upload(h32)
        x = _stage_abc.upload_series_f32(mem, ts, C_alloc, m.detrend_type)
        self._warn_nonfinite(m, x)

        def taper_norms():
            return float(np.abs(h32).sum(axis=1).max()), float(np.sqrt((h32.astype(np.float64) ** 2).sum(axis=1)).min())

        args = (mem, x, h, T, R, C_alloc, C, m.n_time_samples_per_window, m.n_time_samples_per_step, m.n_time_windows, m.n_fft_samples,
                _lib.DETREND[m.detrend_type])
        sp = _stage_abc.spectra_f32(*args, planes_hint, taper_norms=taper_norms)
        if sp.P is not None:
            # the quality check of the format, read at once (Multitaper.device_spectra of the PyTorch host defers it): one scale per
            # channel serves every window, so a channel with samples far outside its usual range keeps complex64
            if not float(mem.download(sp.quality)[0]) * sp.taper_l2_min >= _lib.PLANES_MIN_TYPICAL:
                sp.free()
                sp = _stage_abc.spectra_f32(*args, None)
        return sp

    def spectra_f64(self, multitaper):
        """Stage A of the float64 engine (the reference's default dtype): float64 windows, tapers and transform, complex128
        spectra X[F][W][R][K][C] (_stage_abc.spectra_f64)."""
        m, mem = multitaper, self.memory
        self._series_checks(m, "complex-valued time series: use the PyTorch host (SC_HIP_HOST=torch)")
        ts = np.ascontiguousarray(np.asarray(m.time_series), dtype=np.float64)
        T, R, C = ts.shape
        x = mem.upload(ts)
        h = mem.upload(np.ascontiguousarray(np.asarray(m.tapers, dtype=np.float64).T / m.sampling_frequency, dtype=np.float64))
        self._warn_nonfinite(m, x, f64=True)
        m._finite_checked = True
        return _stage_abc.spectra_f64(mem, x, h, T, R, C, m.n_time_samples_per_window, m.n_time_samples_per_step, m.n_time_windows,
                                      m.n_fft_samples, _lib.DETREND[m.detrend_type])

    def upload_coefficients(self, coef, f64=False):
        """Reference-layout (W, R, K, N, C) complex coefficients -> device spectra that hold all N bins as given
        (_stage_abc.upload_coefficients: the zero pad channel of an odd count in the float32 engine)."""
        return _stage_abc.upload_coefficients(self.memory, coef, f64)

    def _accumulate_record(self, sp, expectation_type, planes, n_freq=None):
        """accumulate() with the record as a DeviceArray: (record, n_observations)."""
        if sp.C > 256 and sp.P is None:
            raise ValueError(f"one launch of the complex64 / float64 stage-B kernels takes n_signals <= 256 (got {sp.C}): Connectivity of this host "
                             "tiles more signals into channel blocks (numpy_api.Connectivity); NumpyHost.accumulate does not")
        if sp.P is not None and not _stage_abc.fused2_takes(sp.desc(expectation_type, n_freq, padded=True), planes):
            raise _lib.HipEngineError("planes-format spectra: this expectation type / plane set needs complex64 spectra "
                                      "(call spectra() without planes_hint)")
        # (Im s)^2 / s/|s| outside the float32 range: a float64 record from a complex128 copy (_stage_abc.amplitude_guard)
        sp = _stage_abc.amplitude_guard(self.memory, sp, planes)
        return _stage_abc.accumulate(self.memory, sp, expectation_type, planes, n_freq)

    def accumulate(self, sp, expectation_type, planes, n_freq=None):
        """Stage B: un-normalised records [n_bins][floats_per_bin] on the device -- float32, or float64 from complex128 spectra
        (the float64 engine: sc_accumulate_f64).  ``n_freq``: accumulate the first n_freq bins only.  Returns (DeviceBuffer, n_bins,
        n_observations)."""
        rec, n_obs = self._accumulate_record(sp, expectation_type, planes, n_freq)
        return rec.buf, rec.shape[0], n_obs

    # ---- stage D through this host (the drivers of _stage_d.py on float32 records) ------------------------------------------------
    def _request(self, time_series, expectation_type, multitaper_kwargs):
        """The Multitaper of a request of the functional interface, checked before anything is allocated on the device."""
        from .transforms import Multitaper
        if expectation_type not in EXPECTATION_AXES:
            raise ValueError(f"Invalid expectation_type '{expectation_type}'. Must be one of: "
                             + ", ".join(f"'{k}'" for k in EXPECTATION_AXES))
        m = Multitaper(time_series, **multitaper_kwargs)
        if np.asarray(m.time_series).shape[2] > 256:
            raise ValueError(f"n_signals <= 256 through NumpyHost's functional interface (got {np.asarray(m.time_series).shape[2]}): "
                             "numpy_api.Connectivity (SC_HIP_HOST=numpy) tiles more signals into channel blocks")
        return m

    def _csm_records(self, time_series, expectation_type, multitaper_kwargs):
        """(spectra geometry, CSM records as a DeviceArray, n_observations, kept axes) of a time series."""
        m = self._request(time_series, expectation_type, multitaper_kwargs)
        # (complex64 spectra, like Connectivity._csm_records of the PyTorch host: these consumers read every bin of the CSM once, at
        #  window lengths and channel counts where the planes format buys nothing)
        sp = self.spectra(m, planes_hint=None)
        accum, n_obs = self._accumulate_record(sp, expectation_type, _lib.PLANE_CSM)
        sp.free()
        axes = EXPECTATION_AXES[expectation_type]
        kept = tuple(n for i, n in enumerate((sp.W, sp.R, sp.K)) if i not in axes)
        return sp, accum, n_obs, kept

    MVAR_MEASURES = {"directed_transfer_function": _lib.MVAR_DTF, "directed_coherence": _lib.MVAR_DC,
                     "partial_directed_coherence": _lib.MVAR_PDC, "generalized_partial_directed_coherence": _lib.MVAR_GPDC,
                     "direct_directed_transfer_function": _lib.MVAR_DDTF}

    def mvar_measures(self, time_series, measures=("directed_transfer_function",), expectation_type="trials_tapers", tolerance=1e-8,
                      max_iterations=60, **multitaper_kwargs):
        """NumPy time series -> {name: array} for the reference's directed measures of the full multivariate model
        (``Connectivity.directed_transfer_function`` ... ``direct_directed_transfer_function``, connectivity.py:1237-1426; out[...,
        i, j] = j -> i on the non-negative bins): cross-spectral records on the device, ONE batched C x C Wilson factorisation
        (sc_mvar_factor_f64, connectivity.py:567-589), one small kernel and one download per measure."""
        unknown = [name for name in measures if name not in self.MVAR_MEASURES]
        if unknown:
            raise ValueError(f"unknown MVAR measures {unknown}; available: {sorted(self.MVAR_MEASURES)}")
        _stage_d.check_max_iterations(max_iterations)
        sp, accum, n_obs, kept = self._csm_records(time_series, expectation_type, multitaper_kwargs)
        C, F, N = sp.C, sp.F, sp.n_fft
        if C > self.lib.sc_mvar_max_signals():
            raise ValueError(f"the full Wilson factorisation supports n_signals <= {self.lib.sc_mvar_max_signals()} (got {C})")
        G, _, _, summary = _stage_d.mvar_factor(self.memory, accum.shape[0] // F, N, C, accum=accum, n_freq_accum=F,
                                                planes=_lib.PLANE_CSM, n_obs=n_obs, tolerance=tolerance, max_iterations=max_iterations)
        self.last_wilson = dict(iterations=int(summary[0]), not_converged=int(summary[1]), cholesky_fallbacks=int(summary[2]))
        return {name: self.memory.download(_stage_d.mvar_measure(self.memory, G, self.MVAR_MEASURES[name])).reshape(kept + (F, C, C))
                for name in measures}

    def global_coherence(self, time_series, max_rank=1, **multitaper_kwargs):
        """NumPy time series -> (values (n_time_windows, n_fft_samples, max_rank), vectors (n_time_windows, n_fft_samples, n_signals,
        max_rank)) like the reference's ``Connectivity.global_coherence`` (connectivity.py:822-895): the leading eigenpairs of the
        cross-spectral matrix of every (window, two-sided bin) (sc_global_coherence_f64); always over trials and tapers."""
        sp, accum, n_obs, kept = self._csm_records(time_series, "trials_tapers", multitaper_kwargs)
        C = sp.C
        max_rank = int(max_rank)
        if not 1 <= max_rank <= min(C, sp.R * sp.K):
            raise ValueError(f"max_rank must be between 1 and min(n_signals, n_trials * n_tapers) = {min(C, sp.R * sp.K)}")
        if C > self.lib.sc_global_coherence_max_signals():
            raise ValueError(f"global_coherence supports n_signals <= {self.lib.sc_global_coherence_max_signals()}")
        values, vectors = _stage_d.global_coherence(self.memory, accum, sp.W, sp.F, sp.n_fft, C, _lib.PLANE_CSM, n_obs, max_rank,
                                                    ascending=max_rank < C - 1)
        return self.memory.download(values), self.memory.download(vectors)

    def pairwise_spectral_granger_prediction(self, time_series, pairs=None, expectation_type="trials_tapers", tolerance=1e-8,
                                             max_iterations=60, **multitaper_kwargs):
        """NumPy time series -> the reference's ``Connectivity.pairwise_spectral_granger_prediction()`` (connectivity.py:
        1161-1213; out[..., i, j] = j -> i, NaN elsewhere) for all channel pairs or the listed ``pairs``: cross-spectral records
        on the device, batched 2 x 2 Wilson factorisations (sc_granger_pairwise_f64), one download."""
        sp, accum, n_obs, kept = self._csm_records(time_series, expectation_type, multitaper_kwargs)
        C, F, N = sp.C, sp.F, sp.n_fft
        if pairs is None:
            pairs = [(i, j) for i in range(C) for j in range(i + 1, C)]
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if ((pairs < 0) | (pairs >= C)).any():
            raise IndexError("pair index outside the signals")
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        _stage_d.check_max_iterations(max_iterations)
        if len(pairs) == 0:
            return np.full(kept + (F, C, C), np.nan)
        out, _, _, summary = _stage_d.granger_pairwise(self.memory, accum, accum.shape[0] // F, F, N, C, _lib.PLANE_CSM, n_obs, pairs,
                                                       tolerance, max_iterations)
        self.last_wilson = dict(not_converged=int(summary[1]), cholesky_fallbacks=int(summary[2]))
        return self.memory.download(out).reshape(kept + (F, C, C))

    def canonical_coherence(self, time_series, group_labels, **multitaper_kwargs):
        """NumPy time series -> (array (n_time_windows, n_frequencies, n_groups, n_groups), sorted labels) like the reference's
        ``Connectivity.canonical_coherence(group_labels)`` (connectivity.py:745-820, 1953-2032; always over trials and tapers)."""
        sp, accum, n_obs, kept = self._csm_records(time_series, "trials_tapers", multitaper_kwargs)
        C, F, n_bins = sp.C, sp.F, accum.shape[0]
        group_labels = np.asarray(group_labels)
        if group_labels.shape != (C,):
            raise ValueError(f"group_labels needs one label per signal ({C}), got shape {group_labels.shape}")
        labels = np.unique(group_labels)
        groups = [np.flatnonzero(group_labels == lab) for lab in labels]
        n_g = len(groups)
        res = np.ones((n_bins, n_g, n_g))
        res[:, np.arange(n_g), np.arange(n_g)] = np.nan
        # (a group with at least as many channels as observations spans the observation space: coherence 1 with every other group)
        small = [k for k, g in enumerate(groups) if len(g) < n_obs]
        max_group = int(self.lib.sc_canonical_max_group())
        if any(len(groups[k]) > max_group for k in small):
            raise ValueError(f"canonical_coherence: the whitening kernel takes up to {max_group} channels per group")
        if len(small) >= 2:
            sub, self.last_canonical_failures = _stage_d.canonical_coherence(self.memory, accum, C, _lib.PLANE_CSM, n_obs,
                                                                             [groups[k] for k in small])
            res[np.ix_(np.arange(n_bins), small, small)] = self.memory.download(sub)
        return res.reshape(sp.W, F, n_g, n_g), labels

    def _planes_expectation(self, m, expectation_type, planes):
        """Would sc_fused2.hip take this request?  (asked BEFORE stage A picks the device format of the spectra)"""
        ts = np.asarray(m.time_series)
        return _stage_abc.planes_request_ok(m.n_time_windows, ts.shape[1], np.asarray(m.tapers).shape[1], m.n_fft_samples,
                                            _lib.padded_channels(ts.shape[2], 256), expectation_type, planes)

    def connectivity(self, time_series, measures=("coherence_magnitude",), expectation_type="trials_tapers", **multitaper_kwargs):
        """NumPy time series (n_time, n_trials, n_signals) -> {measure name: NumPy array} shaped like the reference's
        ``Connectivity.<measure>()`` results (non-negative frequencies)."""
        unknown = [name for name in measures if name not in MEASURES]
        if unknown and expectation_type in EXPECTATION_AXES:           # (an invalid expectation_type is reported first: _request)
            raise ValueError(f"unknown measures {unknown}; available: {sorted(MEASURES)}")
        m = self._request(time_series, expectation_type, multitaper_kwargs)
        planes = 0
        for name in measures:
            planes |= _lib.MEASURE_PLANES[MEASURES[name]]
        # (the planes format holds observations as ONE run of rows: the expectation types that reduce every stored axis but
        #  the frequency, or a contiguous tail of them -- sc_fused2_supported decides; anything else takes complex64)
        sp = self.spectra(m, planes_hint=planes if self._planes_expectation(m, expectation_type, planes) else None)
        rec, n_obs = self._accumulate_record(sp, expectation_type, planes)
        sp.free()
        C, F = sp.C, sp.F
        axes = EXPECTATION_AXES[expectation_type]
        kept = tuple(n for i, n in enumerate((sp.W, sp.R, sp.K)) if i not in axes)
        out = {}
        for name in measures:
            dev = _stage_abc.measure(self.memory, rec, C, planes, n_obs, MEASURES[name], wide=True)
            out[name] = self.download(dev.buf, kept + (F,) + dev.shape[1:], dev.dtype)
            del dev
        del rec
        out["frequencies"] = np.asarray(m.frequencies)[:F].copy()
        if F and out["frequencies"][-1] < 0:
            out["frequencies"][-1] = abs(out["frequencies"][-1])
        out["time"] = np.asarray(m.time)
        return out
