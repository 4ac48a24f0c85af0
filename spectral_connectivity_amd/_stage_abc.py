"""Stages A, B and C: the call sequences every request runs -- the multitaper transform, the accumulation of the records, the
epilogue that turns a record into a measure -- written once for both hosts, next to the stage-D drivers of ``_stage_d.py``.

Same pattern as there: the first argument is the memory adapter ``mem`` (engine.TorchMemory / numpy_host.NumpyMemory), the module
never imports torch, and every returned array is a device array of the host's own type.  Beyond what ``_stage_d.py`` lists, the
drivers here use:

    mem.empty(shape, dtype)              also float32 and complex64
    mem.head(array, n)                   the first n rows of an array, as an array on the same memory
    mem.twiddles(n_fft)                  the exp(-2 pi i m / N) table of the fused transforms (each host caches what make_twiddles gives)
    mem.workspace(n_bytes, owner)        split-bin scratch of stage B, None for 0 bytes -- PyTorch host: the per-device cache, or the
                                         caller's dict ``owner`` (a captured pass); torch-free host: a pool buffer of the call's own
    mem.fft_plan(n_fft, batch, f64)      context manager around ONE execution of a rocFFT plan: the PyTorch host hands out its cached
                                         plan; the torch-free host creates one, synchronises and destroys it
    mem.spectra(X, dims, strides, n_fft, real_input, C_alloc=, P=, scale=)      the host's spectra object (a subclass of Spectra)
    mem.read_scales(spectra)             the 2 C_alloc floats of planes-format spectra's ``scale`` as a NumPy array (one small read-back)

Nothing is released explicitly: the torch-free host's buffers go back to its pool with their last reference (DeviceBuffer.__del__),
which for ``work``, ``y`` and the workspace is the driver's return -- no later than the explicit frees that host had.  No driver reads
anything back or synchronises (the torch-free ``fft_plan`` aside): when the planes format's quality scalar is read stays with the
caller, and the fused complex64 transform and ``accumulate`` with a ``workspace_owner`` remain safe to capture in a hipGraph
(engine.GraphedMeasures).  A new stage-A output format is one more branch of ``spectra_f32``, a new accumulator family one more call
in ``accumulate`` (and its bit in ``_lib``): both hosts get it through their one-line wrappers.
"""
import ctypes
from ctypes import byref, c_int64
from logging import getLogger

import numpy as np

from . import _lib
from ._lib import EXPECTATION_AXES, SpectraDesc
from ._stage_d import _ptr

logger = getLogger(__name__)
DETREND_ERROR = ("Invalid trend type '{}' is not supported.\n"
                 "Valid options are 'linear'/'l', 'constant'/'c' or None.")
NONFINITE_WARNING = ("Input time_series contains NaN or infinite values.\n"
                     "This will produce invalid spectral estimates.")
MAX_KERNEL_SIGNALS = 256          # SC_MAX_SIGNALS of csrc/sc_common.h: what one launch of the stage-B kernels stages per observation row
MEASURE_MULTI_MAX = 4


def check_detrend(detrend_type):
    if detrend_type not in _lib.DETREND:
        raise ValueError(DETREND_ERROR.format(detrend_type))


def dense_strides(W, R, K, C_alloc):
    """(frequency, window, trial, taper) element strides of the dense [F][W][R][K][C_alloc] layout."""
    return (W * R * K * C_alloc, R * K * C_alloc, K * C_alloc, C_alloc)


def spectra_desc(F, W, R, K, n_signals, strides, expectation_type, n_freq=None):
    """The SpectraDesc of spectra [F][W][R][K] x ``n_signals`` (the real count, or the allocated one to have the zero pad channel
    counted as a signal) with the element ``strides`` of (frequency, window, trial, taper), reduced as ``expectation_type`` says."""
    axes = EXPECTATION_AXES[expectation_type]
    sF, sW, sR, sK = strides
    return SpectraDesc(n_freq=F if n_freq is None else n_freq, n_windows=W, n_trials=R, n_tapers=K, n_signals=n_signals,
                       stride_freq=sF, stride_window=sW, stride_trial=sR, stride_taper=sK, reduce_window=int(0 in axes),
                       reduce_trial=int(1 in axes), reduce_taper=int(2 in axes), reserved=0)


def fused2_takes(desc_padded, planes):
    """Does the planes-format stage B (sc_fused2.hip) take ``planes`` for spectra of this (padded) descriptor?"""
    return bool(_lib._handle().sc_fused2_supported(byref(desc_padded), planes))


def planes_request_ok(W, R, K, n_fft, C_alloc, expectation_type, planes):
    """fused2_takes for the dense one-sided spectra stage A would write -- asked BEFORE it picks their device format."""
    return fused2_takes(spectra_desc(n_fft // 2 + 1, W, R, K, C_alloc, dense_strides(W, R, K, C_alloc), expectation_type), planes)


class Spectra:
    """Geometry of device spectra, shared by the hosts' spectra objects (engine.DeviceSpectra, numpy_host.NpSpectra): F, W, R, K, C
    logical sizes, ``C_alloc`` >= C channels stored per row, ``strides`` of (frequency, window, trial, taper) in elements (channel
    stride 1), ``n_fft``, ``real_input``, ``f64`` (complex128 spectra), the planes-format buffers ``P`` / ``scale`` and, when stage A
    wrote that format, ``quality`` -- a device scalar, min over the channels of (typical sample magnitude x channel scale) -- and
    ``taper_l2_min``: their product is the typical coefficient in scaled units, for the caller to hold against _lib.PLANES_MIN_TYPICAL."""

    is_device_spectra = True        # (what Connectivity tests for)

    def __init__(self, X, dims, strides, n_fft, real_input, C_alloc=None, P=None, scale=None, f64=False):
        self._X, self.P, self.scale = X, P, scale
        self.F, self.W, self.R, self.K, self.C = (int(d) for d in dims)
        self.C_alloc = self.C if C_alloc is None else int(C_alloc)
        assert self.C_alloc in (self.C, self.C + 1) and -(-self.C_alloc // 16) == -(-self.C // 16)
        self.strides = tuple(int(s) for s in strides)
        self.n_fft = int(n_fft)
        self.real_input = bool(real_input)   # negative bins are conj mirrors of positive ones
        self.f64 = bool(f64)
        self.quality = self.taper_l2_min = None
        self._amplitude = self._amplitude_scales = self._widened = None      # amplitude_guard: measured / widened once per object

    @property
    def X(self):
        """The complex coefficients (None while only the planes format holds them; engine.DeviceSpectra decodes on first use)."""
        return self._X

    def desc(self, expectation_type, n_freq=None, padded=False):
        """Descriptor of the spectra; ``padded``: with the zero pad channel counted as a signal."""
        return spectra_desc(self.F, self.W, self.R, self.K, self.C_alloc if padded else self.C, self.strides, expectation_type, n_freq)


# ---- stage A ---------------------------------------------------------------------------------------------------------------------
def make_twiddles(mem, n_fft):
    """A fresh exp(-2 pi i m / N) table (what a host's ``mem.twiddles`` caches)."""
    tw = mem.empty((n_fft,), np.complex64)
    _lib.check(_lib._handle().sc_fft_twiddles_f32(n_fft, mem.ptr(tw), mem.stream()), "sc_fft_twiddles_f32")
    return tw


def series_to_f32(mem, xd, T, R, C, C_alloc, detrend_type):
    """(T, R, C) float64 device series -> (T, R, C_alloc) float32: the per-(trial, signal) constant is taken out in float64 BEFORE
    the cast when a detrend is active, and the zero pad channel of an odd count appended."""
    x = mem.empty((T, R, C_alloc), np.float32)
    _lib.check(_lib._handle().sc_timeseries_to_f32(mem.ptr(xd), T, R, C, int(detrend_type is not None), mem.ptr(x), C_alloc,
                                                   mem.stream()), "sc_timeseries_to_f32")
    return x


def upload_series_f32(mem, ts, C_alloc, detrend_type):
    """Host series (T, R, C) -> (T, R, C_alloc) float32 on the device for the float32 engine.  float64: uploaded as it is and
    converted there (series_to_f32); anything else: cast on the host, where an odd channel count also gets its ONE all-zero pad
    channel before the upload."""
    T, R, C = ts.shape
    if ts.dtype == np.float64 and ts.size:
        return series_to_f32(mem, mem.upload(ts), T, R, C, C_alloc, detrend_type)
    xh = np.ascontiguousarray(np.asarray(ts), dtype=np.float32)
    if C_alloc != C:
        xh = np.concatenate([xh, np.zeros(xh.shape[:2] + (1,), dtype=np.float32)], axis=2)
    return mem.upload(xh)


def spectra_f32(mem, x, tapers, T, R, C_alloc, C, L, step, W, N, detrend, planes_hint, mark=None, use_fused=None, taper_norms=None):
    """Stage A of the float32 engine: (T, R, C_alloc) float32 series, (K, L) float32 tapers / fs -> spectra [F][W][R][K][C_alloc].
    Planes format (``_lib.planes_format_applies`` for the families ``planes_hint``): a scan of the series for the channel scales,
    then the fused transform writes the f16 pieces -- the spectra come back with ``quality`` still on the device and
    ``taper_l2_min``; ``taper_norms()`` gives (max_k sum_n |h_k[n]|, min_k ||h_k||_2).  Otherwise complex64: one fused kernel
    (sc_mtfft.hip) for the lengths it has, tapered windows + rocFFT for the others.  ``detrend``: the ``_lib.DETREND`` code."""
    lib, mark = _lib._handle(), mark or (lambda name: None)
    K = int(tapers.shape[0])
    F = N // 2 + 1
    dims, strides = (F, W, R, K, C), dense_strides(W, R, K, C_alloc)
    st = mem.stream()
    if use_fused is None:
        use_fused = bool(lib.sc_multitaper_fft_supported(L, N))
    if use_fused and _lib.planes_format_applies(L, N, C_alloc, planes_hint, spectra_bytes=F * W * R * K * C_alloc * 8):
        P = mem.empty((F * W * R * K * int(lib.sc_planes_row_bytes(C_alloc)),), np.uint8)
        scale = mem.empty((2 * C_alloc,), np.float32)
        work_bytes = int(lib.sc_planes_scales_work_bytes(T * R, C_alloc))
        work = mem.empty((work_bytes,), np.uint8)
        quality = mem.empty((1,), np.float32)
        assert taper_norms is not None, "the planes format needs the caller's taper_norms"
        abs_sum, l2_min = taper_norms()
        _lib.check(lib.sc_planes_scales_quality_f32(mem.ptr(x), T, R, C_alloc, detrend, abs_sum, mem.ptr(scale), mem.ptr(work),
                                                    work_bytes, mem.ptr(quality), st), "sc_planes_scales_quality_f32")
        _lib.check(lib.sc_multitaper_fft_planes_f32(mem.ptr(x), T, R, C_alloc, L, step, W, N, mem.ptr(tapers), K, detrend,
                                                    mem.ptr(mem.twiddles(N)), mem.ptr(scale), mem.ptr(P), st),
                   "sc_multitaper_fft_planes_f32")
        mark("mtfft_fused")
        sp = mem.spectra(None, dims, strides, N, True, C_alloc=C_alloc, P=P, scale=scale)
        sp.quality, sp.taper_l2_min = quality, l2_min
        return sp
    X = mem.empty((F, W, R, K, C_alloc), np.complex64)
    if use_fused:
        # one kernel: window + detrend + taper + FFT + transposed store (sc_mtfft.hip)
        _lib.check(lib.sc_multitaper_fft_f32(mem.ptr(x), T, R, C_alloc, L, step, W, N, mem.ptr(tapers), K, detrend,
                                             mem.ptr(mem.twiddles(N)), mem.ptr(X), st), "sc_multitaper_fft_f32")
        mark("mtfft_fused")
    else:
        batch = W * R * K * C_alloc
        y = mem.empty((batch, N), np.float32)
        _lib.check(lib.sc_taper_windows_f32(mem.ptr(x), T, R, C_alloc, L, step, W, N, mem.ptr(tapers), K, detrend, mem.ptr(y), st),
                   "sc_taper_windows_f32")
        mark("taper_windows")
        with mem.fft_plan(N, batch, False) as plan:
            _lib.check(lib.sc_fft_execute(plan, mem.ptr(y), mem.ptr(X), st), "sc_fft_execute")
        mark("rocfft_r2c")
    return mem.spectra(X, dims, strides, N, True, C_alloc=C_alloc)


def spectra_f64(mem, x, tapers, T, R, C, L, step, W, N, detrend, mark=None, use_fused=None):
    """Stage A of the float64 engine: (T, R, C) float64 series, (K, L) float64 tapers / fs -> complex128 spectra [F][W][R][K][C].
    One fused kernel (sc_multitaper_fft_f64) for the lengths it compiles and grids it can index; sc_taper_windows_f64 +
    double-precision rocFFT + transpose for any other."""
    lib, mark = _lib._handle(), mark or (lambda name: None)
    K = int(tapers.shape[0])
    F = N // 2 + 1
    st = mem.stream()
    if use_fused is None:
        use_fused = bool(lib.sc_multitaper_fft_f64_supported(L, N)) and R <= 65535 and W <= 65535
    X = mem.empty((F, W, R, K, C), np.complex128)
    if use_fused:
        _lib.check(lib.sc_multitaper_fft_f64(mem.ptr(x), T, R, C, L, step, W, N, mem.ptr(tapers), K, detrend, mem.ptr(X), st),
                   "sc_multitaper_fft_f64")
        mark("mtfft_fused_f64")
    else:
        batch = W * R * K * C
        y = mem.empty((batch, N), np.float64)
        _lib.check(lib.sc_taper_windows_f64(mem.ptr(x), T, R, C, L, step, W, N, mem.ptr(tapers), K, detrend, mem.ptr(y), st),
                   "sc_taper_windows_f64")
        mark("taper_windows_f64")
        with mem.fft_plan(N, batch, True) as plan:
            _lib.check(lib.sc_fft_execute_f64(plan, mem.ptr(y), mem.ptr(X), st), "sc_fft_execute_f64")
        mark("rocfft_d2z")
    return mem.spectra(X, (F, W, R, K, C), dense_strides(W, R, K, C), N, True)


def upload_coefficients(mem, coef, f64):
    """Reference-layout (W, R, K, N, C) complex coefficients -> spectra that hold all N bins as given; the float32 engine appends
    the zero pad channel of an odd count (up to the 256 signals one launch of the complex64 kernels takes)."""
    coef = np.asarray(coef)
    W, R, K, N, C = coef.shape
    Ca = C if f64 else _lib.padded_channels(C, MAX_KERNEL_SIGNALS)
    coef = np.ascontiguousarray(coef, dtype=np.complex128 if f64 else np.complex64)
    if Ca != C:
        coef = np.concatenate([coef, np.zeros(coef.shape[:-1] + (1,), dtype=np.complex64)], axis=-1)
    return mem.spectra(mem.upload(coef), (N, W, R, K, C), (Ca, R * K * N * Ca, K * N * Ca, N * Ca), N, False, C_alloc=Ca)


def decode_planes(mem, sp):
    """complex64 coefficients [F][W][R][K][C_alloc] of planes-format spectra (lossless up to the format's 22 bits)."""
    X = mem.empty((sp.F, sp.W, sp.R, sp.K, sp.C_alloc), np.complex64)
    d = sp.desc("trials_tapers", padded=True)
    _lib.check(_lib._handle().sc_spectra_from_planes_f32(mem.ptr(sp.P), byref(d), mem.ptr(sp.scale), mem.ptr(X), mem.stream()),
               "sc_spectra_from_planes_f32")
    return X


# ---- amplitude range of the float32 engine -----------------------------------------------------------------------------------------
# Two accumulator families form quantities a float32 number cannot hold for coefficients x far from 1.  (Im s)^2 is of the order
# |x_i|^2 |x_j|^2: float32's smallest normal number is 2^-126, so a product d = Im s with |d| < 2^-63 has a square that is subnormal or
# 0 -- and no float32 RECORD can hold the sum either, whatever the kernel does.  Let t_c be the root mean square of channel c's
# coefficients.  The products of a pair spread around t_i t_j; one 2^8 times smaller contributes 2^-16 of a typical term to the sum
# of squares, far below the 1e-5 the records are held to, so only products down to 2^-8 t_i t_j need a normal square:
# t_i t_j >= 2^(-63 + 8) = 2^-55 for every pair, i.e. for the two quietest live channels.  At the other end squares overflow from
# |d| = 2^64; with 2^10 for the sum over up to a million observations the two largest coefficients must satisfy m_i m_j <= 2^54.
# s / |s| is formed from the unit phasors x / |x| of the factors (every route), whose |x|^2 must stay normal: coefficients down
# to 2^-12 of the typical one (one in 2^24 for Gaussian data) need |x| >= 2^-63, so t_c >= 2^-51; and m_c <= 2^60 keeps |x|^2 finite.
# Volts (1e-6) and 24-bit ADC counts are far inside; tesla (1e-13) is outside for (Im s)^2 and inside for s / |s|.
IM_SQ_MIN_PAIR_TYPICAL, IM_SQ_MAX_PAIR_LARGEST = 2.0 ** -55, 2.0 ** 54
UNIT_MIN_TYPICAL, UNIT_MAX_LARGEST = 2.0 ** -51, 2.0 ** 60
# Planes format: the kernel sums (Im s)^2 of the SCALED coefficients x * scale[c] (typical size >= 2.5 by the format's quality check, at
# most 2^12: sc_fused2.hip) and multiplies the sum by (inv_i inv_j)^2, inv = 1 / scale, on the way out.  Nothing is estimated: the
# factor itself must be a normal float32, (inv_i inv_j)^2 >= 2^-124, i.e. inv_i inv_j >= 2^-62 for the two smallest; and the largest
# entry, at most n_obs 2^50 (inv_i inv_j)^2, must stay finite: inv_i inv_j <= 2^28 covers 2^20 observations per bin.
PLANES_MIN_PAIR_INVERSE, PLANES_MAX_PAIR_INVERSE = 2.0 ** -62, 2.0 ** 28
SQUARING_PLANES = _lib.PLANE_IM_SQ | _lib.PLANE_UNIT


def _span(sp):
    """Elements from the first to the last coefficient of the spectra (their rows are dense: every stride a multiple of C_alloc)."""
    return sum((n - 1) * st for n, st in zip((sp.F, sp.W, sp.R, sp.K), sp.strides)) + sp.C_alloc


def amplitude_range(mem, sp):
    """(typical, largest) coefficient magnitude per channel of complex64 spectra, NumPy float64 [C]: the root mean square and the
    largest |Re|, |Im| from one reduction over them (sc_amplitude_range_f32).  One small read-back, kept on the spectra object."""
    if sp._amplitude is None:
        lib = _lib._handle()
        X = sp.X
        assert all(st % sp.C_alloc == 0 for st in sp.strides), "the amplitude scan needs spectra whose rows are dense"
        n_rows = _span(sp) // sp.C_alloc
        work_bytes = int(lib.sc_amplitude_range_work_bytes(n_rows, sp.C_alloc))
        work, out = mem.empty((work_bytes,), np.uint8), mem.empty((2, sp.C_alloc), np.float64)
        _lib.check(lib.sc_amplitude_range_f32(mem.ptr(X), n_rows, sp.C_alloc, mem.ptr(out), mem.ptr(work), work_bytes,
                                              mem.stream()), "sc_amplitude_range_f32")
        both = np.asarray(mem.download(out), dtype=np.float64).reshape(2, sp.C_alloc)[:, :sp.C]
        sp._amplitude = (np.sqrt(both[0] / n_rows), both[1])
    return sp._amplitude


def amplitude_out_of_range(typical, largest, planes):
    """Why the float32 kernels cannot take ``planes`` for channels of these magnitudes (a sentence), or None.  Silent channels
    (all zero: every product is an exact 0) and channels with NaN / infinite coefficients (non-finite on either engine) do not count."""
    live = np.isfinite(typical) & np.isfinite(largest) & (typical > 0)
    t, m = np.sort(typical[live]), np.sort(largest[live])
    if planes & _lib.PLANE_IM_SQ and t.size >= 2:
        if t[0] * t[1] < IM_SQ_MIN_PAIR_TYPICAL:
            return (f"(Im s)^2 of the two quietest channels (typical coefficients {t[0]:.3g}, {t[1]:.3g}) is below the float32 range")
        if m[-1] * m[-2] > IM_SQ_MAX_PAIR_LARGEST:
            return (f"(Im s)^2 of the two largest channels (coefficients up to {m[-1]:.3g}, {m[-2]:.3g}) is above the float32 range")
    if planes & _lib.PLANE_UNIT and t.size >= 1:
        if t[0] < UNIT_MIN_TYPICAL:
            return f"|x|^2 of the quietest channel (typical coefficient {t[0]:.3g}) is below the float32 range"
        if m[-1] > UNIT_MAX_LARGEST:
            return f"|x|^2 of the largest channel (coefficients up to {m[-1]:.3g}) is above the float32 range"
    return None


def planes_scales_out_of_range(inverse, planes):
    """The same question for spectra only the planes format holds, from the reciprocals of its channel scales (derivation above)."""
    inv = np.sort(inverse[np.isfinite(inverse) & (inverse > 0)])
    if planes & _lib.PLANE_IM_SQ and inv.size >= 2:
        if inv[0] * inv[1] < PLANES_MIN_PAIR_INVERSE:
            return f"the factor that unscales (Im s)^2 of the two quietest channels (1 / scale {inv[0]:.3g}, {inv[1]:.3g}) is below the float32 range"
        if inv[-1] * inv[-2] > PLANES_MAX_PAIR_INVERSE:
            return f"(Im s)^2 of the two largest channels (1 / scale {inv[-1]:.3g}, {inv[-2]:.3g}) is above the float32 range"
    return None


def amplitude_verdict(mem, sp, planes):
    """Why this float32 request must be accumulated in float64 (a sentence), or None; nothing is measured for a request without
    (Im s)^2 or s / |s|, or for complex128 spectra.  The measurement is kept on the spectra object, the verdict is per request."""
    if sp.f64 or not planes & SQUARING_PLANES:
        return None
    if sp._X is None and not planes & _lib.PLANE_UNIT:
        if sp._amplitude_scales is None:
            sp._amplitude_scales = np.asarray(mem.read_scales(sp), dtype=np.float64).reshape(-1)[sp.C_alloc:sp.C_alloc + sp.C]
        return planes_scales_out_of_range(sp._amplitude_scales, planes)
    return amplitude_out_of_range(*amplitude_range(mem, sp), planes)


def widen(mem, sp):
    """complex128 spectra with the values of complex64 (or planes-format) ones: same geometry, the float64 engine's kernels apply."""
    X = sp._X if sp._X is not None else decode_planes(mem, sp)
    n = _span(sp)
    shape = getattr(X, "shape", None)              # (a tensor keeps its five axes: the channel-block tiling gathers along the last)
    Xw = mem.empty(tuple(shape) if shape is not None and int(np.prod(shape)) == n else (n,), np.complex128)
    _lib.check(_lib._handle().sc_spectra_widen_f32(mem.ptr(X), n, mem.ptr(Xw), mem.stream()), "sc_spectra_widen_f32")
    return mem.spectra(Xw, (sp.F, sp.W, sp.R, sp.K, sp.C), sp.strides, sp.n_fft, sp.real_input, C_alloc=sp.C_alloc)


def amplitude_guard(mem, sp, planes, decided=None):
    """The spectra a float32-engine request for ``planes`` is accumulated from: ``sp`` itself while the families that square products
    ((Im s)^2, s / |s|) stay inside the float32 range for its channels (thresholds above) -- in-range data never leave the float32
    kernels --, otherwise a complex128 copy (made once, kept on ``sp``), from which stage B writes a float64 record with the float64
    engine's kernels; one line is logged.  Every consumer of records takes either kind.  The verdict is taken per request: a later
    request that is in range runs on ``sp`` again.  ``decided``: the verdict of a GROUP of processes (True: widen), taken by the
    caller so that every rank accumulates the same kind of record; None: this process decides for itself.  The hosts call this
    before stage B (engine.accumulate, NumpyHost._accumulate_record); ``accumulate`` below takes the spectra as they come."""
    if sp.f64 or not planes & SQUARING_PLANES:
        return sp
    if decided is None:
        why = amplitude_verdict(mem, sp, planes)
        decided = why is not None
    else:
        why = "(Im s)^2 or |x|^2 is outside the float32 range on a process of the group"
    if not decided:
        return sp
    if sp._widened is None:
        sp._widened = widen(mem, sp)
    logger.warning("spectral_connectivity_amd: %s: this request is accumulated by the float64 engine", why)
    return sp._widened


# ---- stage B ---------------------------------------------------------------------------------------------------------------------
def accum_layout(sp, expectation_type, planes, n_freq=None):
    """(n_bins, floats per bin, n_groups, n_observations) of the record of ``planes``."""
    d = sp.desc(expectation_type, n_freq)
    n_bins, fpb, n_groups, n_obs = c_int64(), c_int64(), c_int64(), c_int64()
    _lib.check(_lib._handle().sc_accum_layout(byref(d), planes, byref(n_bins), byref(fpb), byref(n_groups), byref(n_obs)),
               "sc_accum_layout")
    return n_bins.value, fpb.value, n_groups.value, n_obs.value


def accumulate(mem, sp, expectation_type, planes, n_freq=None, which=None, out=None, fold=True, workspace_owner=None, use_fused=None,
               mark=None):
    """Stage B: (un-normalised records [n_bins, floats_per_bin], n_observations) -- float32, float64 from complex128 spectra, into
    ``out`` when the caller brings the record.  ``which`` (float64 engine): the families of ``planes`` to compute, the others are in
    ``out`` already.  ``fold=False`` (planes format, no ``out``): where the kernel split every bin over several workgroups their
    partial records are kept -- the result is then 3-D, [n_parts, n_bins, floats_per_bin], parts in the order their sum is taken.
    ``use_fused=False``: every plane through its separate kernel.  At most 256 signals, or planes-format spectra of a family their
    kernels take: the callers see to that, and to the amplitude range of the float32 kernels (amplitude_guard)."""
    lib, mark = _lib._handle(), mark or (lambda name: None)
    d = sp.desc(expectation_type, n_freq)
    n_bins, fpb, _, n_obs = accum_layout(sp, expectation_type, planes, n_freq)
    st = mem.stream()
    if sp.f64:
        # float64 engine: fp64 matrix cores for the CSM planes, fp64 VALU for the others, double records
        accum = mem.empty((n_bins, fpb), np.float64) if out is None else out
        which = planes if which is None else which
        if which:
            _lib.check(lib.sc_accumulate_f64(mem.ptr(sp.X), byref(d), planes, which, mem.ptr(accum), st), "sc_accumulate_f64")
        mark("accumulate_f64")
        return accum, n_obs
    dp = sp.desc(expectation_type, n_freq, padded=True)
    if sp.P is not None and use_fused is not False and fused2_takes(dp, planes):
        # planes format: CSM (+ |Im s|) straight from the f16 pieces stage A wrote (sc_fused2.hip)
        ws_bytes = int(lib.sc_fused_workspace_bytes(byref(dp), planes))
        part_bytes = n_bins * fpb * 4
        if not fold and ws_bytes >= part_bytes and out is None:
            # partial records kept: parts 1 .. behind part 0 in one allocation of the caller's own
            max_parts = 1 + ws_bytes // part_bytes
            parts = mem.empty((max_parts, n_bins, fpb), np.float32)
            n_parts = ctypes.c_int(1)
            _lib.check(lib.sc_fused2_csm_absim_parts_f32(mem.ptr(sp.P), byref(dp), mem.ptr(sp.scale), planes, mem.ptr(parts),
                                                         mem.ptr(parts, 1), (max_parts - 1) * part_bytes, byref(n_parts), st),
                       "sc_fused2_csm_absim_parts_f32")
            mark("fused2_csm_absim")
            return mem.head(parts, n_parts.value), n_obs
        ws = mem.workspace(ws_bytes, workspace_owner)
        accum = mem.empty((n_bins, fpb), np.float32) if out is None else out
        _lib.check(lib.sc_fused2_csm_absim_f32(mem.ptr(sp.P), byref(dp), mem.ptr(sp.scale), planes, mem.ptr(accum), _ptr(mem, ws),
                                               ws_bytes, st), "sc_fused2_csm_absim_f32")
        mark("fused2_csm_absim")
        return accum, n_obs
    accum = mem.empty((n_bins, fpb), np.float32) if out is None else out
    per_plane_only = use_fused is False        # explicit request (tests): every plane through its separate kernel
    if use_fused is None:
        use_fused = bool(lib.sc_fused_supported(sp.C_alloc))
    # planes the one-pass kernels fill for this shape (sc_fused.hip): CSM, |Im s|, s/|s|; for few channels also
    # (Im s)^2 and sign(Im s).  Whatever is left goes to the per-plane VALU kernel.  The one-pass kernels see the zero
    # pad channel of an odd channel count as a signal (descriptor ``dp``): same record (DeviceSpectra).
    one_pass = int(lib.sc_fused_planes_covered(byref(dp), planes)) if use_fused else 0
    X = mem.ptr(sp.X)
    if one_pass:
        ws_bytes = int(lib.sc_fused_workspace_bytes(byref(dp), planes))
        ws = mem.workspace(ws_bytes, workspace_owner)
        ws_ptr = _ptr(mem, ws)
        if one_pass & _lib.PLANE_CSM:
            # CSM (+ the per-observation |Im s| products, + (Im s)^2): bf16 matrix pipe, or the f32 VALU kernel
            _lib.check(lib.sc_fused_csm_absim_ws_f32(X, byref(dp), planes, mem.ptr(accum), ws_ptr, ws_bytes, st),
                       "sc_fused_csm_absim_ws_f32")
            mark("fused_csm_absim")
        if one_pass & _lib.PLANE_SIGN_IM:
            _lib.check(lib.sc_fused_sign_ws_f32(X, byref(dp), planes, mem.ptr(accum), ws_ptr, ws_bytes, st), "sc_fused_sign_ws_f32")
            mark("fused_sign")
        if one_pass & _lib.PLANE_UNIT:
            # sum s/|s| = the CSM of the unit phasors x/|x|: the same kernels on normalised rows
            sb = int(lib.sc_fused_unit_scratch_bytes(byref(dp)))
            scratch = mem.empty((sb,), np.uint8) if sb else None
            _lib.check(lib.sc_fused_unit_ws_f32(X, byref(dp), planes, mem.ptr(accum), ws_ptr, ws_bytes, _ptr(mem, scratch), sb, st),
                       "sc_fused_unit_ws_f32")
            mark("fused_unit")
        nl = planes & ~one_pass
    else:
        if planes & _lib.PLANE_CSM:
            _lib.check(lib.sc_csm_accumulate_f32(X, byref(d), planes, mem.ptr(accum), st), "sc_csm_accumulate_f32")
            mark("csm_mfma")
        nl = planes & ~_lib.PLANE_CSM
        if nl & _lib.PLANE_UNIT and not per_plane_only:
            # sum s/|s| as the CSM of a normalised copy of the spectra (f32 MFMA) instead of a per-pair rsqrt on the VALU
            sb = int(lib.sc_unit_scratch_bytes(byref(d)))
            scratch = mem.empty((sb,), np.uint8)
            _lib.check(lib.sc_unit_accumulate_f32(X, byref(d), planes, mem.ptr(accum), mem.ptr(scratch), sb, st),
                       "sc_unit_accumulate_f32")
            nl &= ~_lib.PLANE_UNIT
            mark("unit_mfma")
    if nl:
        _lib.check(lib.sc_nonlinear_accumulate_f32(X, byref(d), planes, nl, mem.ptr(accum), st), "sc_nonlinear_accumulate_f32")
        mark("nonlinear_valu")
    return accum, n_obs


# ---- stage C ---------------------------------------------------------------------------------------------------------------------
def measure_output(n_bins, n_signals, which, wide):
    """(shape, NumPy dtype) of one measure over ``n_bins`` bins -- the one table of it: power per signal, the complex-valued
    measures, the real-valued rest per signal pair; ``wide``: float64 / complex128 instead of float32 / complex64."""
    real_t, cplx_t = (np.float64, np.complex128) if wide else (np.float32, np.complex64)
    if which == _lib.M_POWER:
        return (n_bins, n_signals), real_t
    return (n_bins, n_signals, n_signals), (cplx_t if which in _lib.COMPLEX_MEASURES else real_t)


def measure(mem, record, n_signals, planes, n_obs, which, wide, parts=None, out=None):
    """Stage C: one measure from the record [n_bins, floats_per_bin] (after any cross-GPU sum).  ``parts``: contiguous partial
    records [n_parts > 1, n_bins, floats_per_bin] with ``record`` their first -- the epilogue sums them in part order while it
    reads (sc_measure_parts: every measure, power and the complex-valued ones included)."""
    lib = _lib._handle()
    n_bins = record.shape[0]
    if out is None:
        out = mem.empty(*measure_output(n_bins, n_signals, which, wide))
    rec_planes = _lib.record_planes(planes, mem.is_f64(record))
    if parts is not None:
        _lib.check(lib.sc_measure_parts(mem.ptr(parts), mem.ptr(parts, 1), parts.shape[0], parts.shape[1] * parts.shape[2], n_bins,
                                        n_signals, rec_planes, n_obs, which, mem.ptr(out), int(bool(wide)), mem.stream()),
                   "sc_measure_parts")
        return out
    fn = lib.sc_measure_f64 if wide else lib.sc_measure_f32
    _lib.check(fn(mem.ptr(record), n_bins, n_signals, rec_planes, n_obs, which, mem.ptr(out), mem.stream()), "sc_measure")
    return out


def one_launch(which, from_parts):
    """Does the one-launch epilogue take the measures ``which``?  Real-valued C x C ones only, at most four -- and at least two
    (from partial records: one), below which a single call is the same work."""
    simple = all(w != _lib.M_POWER and w not in _lib.COMPLEX_MEASURES for w in which)
    return simple and (1 if from_parts else 2) <= len(which) <= MEASURE_MULTI_MAX


def measure_multi(mem, record, n_signals, planes, n_obs, which, wide, parts=None, outs=None):
    """Stage C for several measures of one record: ONE launch reads the record once (sc_measure_multi_*) where one_launch() says
    so, into ``outs`` when the caller brings them; otherwise one measure() per entry of ``which`` (``parts`` is then None: the
    caller folded them)."""
    which = list(which)
    if not one_launch(which, parts is not None):
        assert parts is None
        return [measure(mem, record, n_signals, planes, n_obs, w, wide) for w in which]
    lib = _lib._handle()
    n_bins, C = record.shape[0], n_signals
    if outs is None:
        outs = [mem.empty((n_bins, C, C), np.float64 if wide else np.float32) for _ in which]
    ids = (ctypes.c_int * len(which))(*which)
    ptrs = (ctypes.c_void_p * len(which))(*[mem.ptr(o).value for o in outs])
    rec_planes = _lib.record_planes(planes, mem.is_f64(record))
    if parts is not None:
        _lib.check(lib.sc_measure_multi_parts(mem.ptr(parts), mem.ptr(parts, 1), parts.shape[0], parts.shape[1] * parts.shape[2],
                                              n_bins, C, rec_planes, n_obs, len(which), ids, ptrs, int(bool(wide)), mem.stream()),
                   "sc_measure_multi_parts")
        return outs
    fn = lib.sc_measure_multi_f64 if wide else lib.sc_measure_multi_f32
    _lib.check(fn(mem.ptr(record), n_bins, C, rec_planes, n_obs, len(which), ids, ptrs, mem.stream()), "sc_measure_multi")
    return outs
