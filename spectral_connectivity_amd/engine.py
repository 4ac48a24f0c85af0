"""Device pipeline glue: torch owns HBM buffers and streams, libsc_hip.so does the work.

Nothing here computes on the CPU: every function launches HIP kernels / rocFFT through the
C ABI (include/sc_hip.h) on the current torch stream and returns device tensors.

The call sequences live in _stage_abc.py (stages A to C) and _stage_d.py, once for this host and the torch-free one.  Here is the
PyTorch host's side of them: the memory adapter ``TorchMemory`` (tensors, the current stream, the plan / twiddle / workspace caches),
``DeviceSpectra``, and public functions that are one call into a driver plus this host's tensor arithmetic -- the pad-channel copy of
a device series, ``row_multiple`` / ``have`` around stage B, the tiling of more than 256 signals, partial records, ``GraphedMeasures``.
"""
import collections
import contextlib
from ctypes import byref, c_void_p

import numpy as np
import torch

from . import _lib, _stage_abc, _stage_d

_plan_cache = collections.OrderedDict()     # (N, batch, device, f64) -> sc_fft_plan handle, least recently used first
PLAN_CACHE_SIZE = 4                          # every plan owns a rocFFT work buffer and up to 64 MB of transform scratch
_twiddle_cache = {}


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr())


def to_host(t):
    """Device tensor -> NumPy array through a page-locked buffer (the caching host allocator keeps and reuses the
    blocks): a pageable copy of a large result runs at ~6 GB/s, a pinned one at link rate.  The array owns its
    buffer (it is the pinned tensor's memory, kept alive by the array)."""
    t = t.contiguous()
    n_bytes = t.numel() * t.element_size()
    if (1 << 20) <= n_bytes <= (2 << 30):
        try:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            torch.cuda.current_stream(t.device).synchronize()
            return h.numpy()
        except RuntimeError:
            pass
    return t.cpu().numpy()


def fft_plan(n_fft, batch, f64=False):
    """rocFFT real-forward plan: rows [batch][N] in, frequency-major [F][batch] out.  A small LRU keeps the plans of
    the last few (N, batch, device, precision) shapes; an evicted plan is destroyed after the device has drained (its
    scratch may still be in use by queued work), so a sweep over window lengths does not pile up plan buffers."""
    key = (int(n_fft), int(batch), torch.cuda.current_device(), bool(f64))
    plan = _plan_cache.get(key)
    if plan is not None:
        _plan_cache.move_to_end(key)
        return plan
    lib = _lib.load()
    while len(_plan_cache) >= PLAN_CACHE_SIZE:
        _, old = _plan_cache.popitem(last=False)
        torch.cuda.synchronize()
        lib.sc_fft_plan_destroy(old)
    handle = c_void_p()
    create = lib.sc_fft_plan_create_f64 if f64 else lib.sc_fft_plan_create
    _lib.check(create(byref(handle), n_fft, batch), "sc_fft_plan_create")
    _plan_cache[key] = handle
    return handle


def clear_plan_cache():
    lib = _lib.load()
    if _plan_cache:
        torch.cuda.synchronize()
    for plan in _plan_cache.values():
        lib.sc_fft_plan_destroy(plan)
    _plan_cache.clear()


class DeviceSpectra(_stage_abc.Spectra):
    """One-sided (or caller-described) Fourier coefficients resident in HBM (geometry and ``desc``: _stage_abc.Spectra).

    ``X`` is a complex64 tensor (float32 engine) or a complex128 tensor (float64 engine, ``f64``: no pad channel,
    every consumer takes the fp64 kernels of sc_f64.hip); ``dims`` = (F, W, R, K, C) logical sizes and ``strides`` =
    element strides of (freq, window, trial, taper) -- channel stride is 1.  ``C_alloc`` >= C channels are
    stored per row: an odd channel count gets one all-zero channel appended, so that rows stay 16-byte
    aligned and the one-pass stage-B kernels (even channel counts) apply; a record accumulated over C_alloc
    channels IS the record of the first C (same 16 x 16 tiling, the extra row / column lies in tile padding).

    Planes format (float32 engine, round 4): ``P`` holds the same coefficients as two f16 pieces per real number
    (x * scale[c] = h + m, dense rows [F][W][R][K] of sc_planes_row_bytes(C) bytes: sc_fused2.hip) and ``scale`` the
    per-channel powers of two (then their reciprocals).  Stage A can write it instead of complex64 (same volume); the
    CSM / |Im s| accumulation then runs on it directly, and ``X`` is decoded from it on first use by anything else.
    """

    def __init__(self, X, dims, strides, n_fft, real_input, C_alloc=None, P=None, scale=None):
        super().__init__(X, dims, strides, n_fft, real_input, C_alloc, P, scale, f64=X is not None and X.dtype == torch.complex128)
        self.device = X.device if X is not None else P.device

    def planes_typical_coefficient(self):
        """Smallest typical coefficient over the channels, in the scaled units of the f16 pieces (one small read-back)."""
        return float(self.quality.item()) * self.taper_l2_min

    @property
    def X(self):
        """The complex64 / complex128 coefficients; decoded from the planes format (lossless up to its 22 bits) on first use."""
        if self._X is None:
            self._X = _stage_abc.decode_planes(TorchMemory(self.device), self)
        return self._X

    def coefficients(self):
        """The spectra as a (F, W, R, K, C) tensor view of a contiguous X (the zero pad channel dropped)."""
        return self.X.view(self.F, self.W, self.R, self.K, self.C_alloc)[..., :self.C]

    def freq_slice(self, f0, f1):
        """The bins [f0, f1) as a view (no copy): same strides, pointer advanced by f0 * stride_freq."""
        assert 0 <= f0 < f1 <= self.F
        P = flat = None
        if self.P is not None:
            per_bin = self.W * self.R * self.K * int(_lib.load().sc_planes_row_bytes(self.C_alloc))
            P = self.P[f0 * per_bin:f1 * per_bin]
        if self._X is not None:
            assert self._X.is_contiguous()
            flat = self._X.view(-1)[f0 * self.strides[0]:]
        return DeviceSpectra(flat, (f1 - f0, self.W, self.R, self.K, self.C), self.strides, self.n_fft,
                             self.real_input, C_alloc=self.C_alloc, P=P, scale=self.scale)


def _taper_norms(tapers_over_fs):
    """(max_k sum_n |h_k[n]|, min_k ||h_k||_2): the bound behind the channel scales of the planes format and the size of a typical
    coefficient per unit of sample spread -- properties of the tapers, kept ON the tensor object together with its version
    counter: one device synchronisation per taper tensor, not per transform."""
    cached = getattr(tapers_over_fs, "_sc_norms", None)
    if cached is None or cached[1] != tapers_over_fs._version:
        both = torch.stack([tapers_over_fs.abs().sum(dim=1).max(), tapers_over_fs.pow(2).sum(dim=1).sqrt().min()]).tolist()
        cached = ((float(both[0]), float(both[1])), tapers_over_fs._version)
        tapers_over_fs._sc_norms = cached
    return cached[0]


def twiddles(n_fft, device):
    """exp(-2 pi i m / N) table for the fused FFT kernel (device, cached per (N, device))."""
    key = (int(n_fft), str(device))
    tw = _twiddle_cache.get(key)
    if tw is None:
        tw = _twiddle_cache[key] = _stage_abc.make_twiddles(TorchMemory(device), n_fft)
    return tw


_ws_cache = {}


def _workspace(n_bytes, device, owner=None):
    """Scratch the fused stage-B kernel uses to split bins over workgroups (kept and reused per device).  ``owner``: a dict of
    the caller's in which the buffer lives instead of the per-device cache -- a captured pass (GraphedMeasures) replays the
    buffer's ADDRESS, so it must not be the shared one, which a later, larger request replaces and frees."""
    if n_bytes <= 0:
        return None
    cache = _ws_cache if owner is None else owner
    key = (device.type, device.index)
    buf = cache.get(key)
    if buf is None or buf.numel() < n_bytes:
        buf = torch.empty(n_bytes, dtype=torch.uint8, device=device)
        cache[key] = buf
    return buf


_TORCH_DTYPES = {np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64,
                 np.complex64: torch.complex64, np.complex128: torch.complex128}
_TORCH_DTYPES.update({np.dtype(k): v for k, v in list(_TORCH_DTYPES.items())})


class TorchMemory:
    """The memory adapter of the shared drivers (_stage_abc.py, _stage_d.py) on this host: tensors of ``device``, calls on the
    current stream."""

    def __init__(self, device):
        self.device = device

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=_TORCH_DTYPES[dtype], device=self.device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=_TORCH_DTYPES[dtype], device=self.device)

    def upload(self, array):
        return torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def ptr(self, t, first_row=0):
        return c_void_p(t.data_ptr() + (first_row * t.stride(0) * t.element_size() if first_row else 0))

    stream = staticmethod(_stream)
    download = staticmethod(to_host)
    spectra = DeviceSpectra

    def is_f64(self, record):
        return record.dtype == torch.float64

    def read_scales(self, spectra):
        return spectra.scale.cpu().numpy()

    def fill_nan(self, t):
        t.fill_(float("nan"))

    def read_int(self, t):
        return int(t.item())

    def hstack(self, chunks, n_rows):
        return chunks[0] if len(chunks) == 1 else torch.cat([c.view(n_rows, -1) for c in chunks], dim=1).reshape(-1)

    def head(self, t, n):
        return t[:n]

    def twiddles(self, n_fft):
        return twiddles(n_fft, self.device)

    def workspace(self, n_bytes, owner=None):
        return _workspace(n_bytes, self.device, owner)

    @contextlib.contextmanager
    def fft_plan(self, n_fft, batch, f64=False):
        yield fft_plan(n_fft, batch, f64)       # (cached: nothing to wait for or destroy)


def multitaper_spectra(x, tapers_over_fs, n_window, n_step, n_fft, n_windows, detrend_type, mark=None,
                       use_fused=None, n_signals=None, planes_hint=None):
    """Stage A on device: (T,R,C) float32 tensor -> DeviceSpectra [F][W][R][K][C] (_stage_abc.spectra_f32).

    ``tapers_over_fs``: (K, L) float32 device tensor = reference tapers^T / fs
    (folds the sqrt(fs) of transforms.py:1440 and the /fs of transforms.py:1405).
    ``n_signals``: number of real channels when ``x`` already carries the all-zero pad channel of an odd channel count
    (appended on the host before the upload, transforms.Multitaper.device_spectra); a device tensor with an odd channel
    count that arrives unpadded is copied into a padded buffer here (one strided device copy).
    ``planes_hint``: the accumulator families the caller will ask for.  Any family sc_fused2.hip serves, 44 ... 1024 signals, a
    window length stage A has the output for (the powers of two 64 ... 4096, the lengths 200 ... 2000 of sc_mtfft_mixed.hip:
    sc_multitaper_fft_planes_supported) and at least 256 MB of spectra (_lib.planes_format_applies): the spectra are
    written in the planes format (two f16 pieces per real number) -- a scan of the series for the channel scales, then the same
    fused transform.  The scan also reports how large a typical coefficient will be in the format's scaled units
    (``DeviceSpectra.planes_typical_coefficient()``): one scale per channel serves every window, so the format is meant for
    series without samples hundreds of times the typical amplitude; Multitaper.device_spectra checks against
    _lib.PLANES_MIN_TYPICAL and re-runs the transform into complex64 otherwise.
    """
    T, R, C_real = x.shape
    if n_signals is not None:
        assert n_signals in (C_real, C_real - 1)
        C_real = int(n_signals)
    elif _lib.padded_channels(C_real, _lib.PLANES_FORMAT_MAX_CHANNELS) != C_real:
        padded = torch.zeros((T, R, C_real + 1), dtype=x.dtype, device=x.device)
        padded[..., :C_real].copy_(x)                # odd channel count: one zero channel (see DeviceSpectra)
        x = padded
    T, R, C = x.shape
    K, L = tapers_over_fs.shape
    assert L == n_window
    return _stage_abc.spectra_f32(TorchMemory(x.device), x, tapers_over_fs, T, R, C, C_real, L, n_step, n_windows, n_fft,
                                  _lib.DETREND[detrend_type], planes_hint, mark, use_fused,
                                  taper_norms=lambda: _taper_norms(tapers_over_fs))


def multitaper_spectra_f64(x, tapers_over_fs, n_window, n_step, n_fft, n_windows, detrend_type, mark=None, use_fused=None):
    """Stage A of the float64 engine: (T,R,C) float64 tensor -> complex128 DeviceSpectra [F][W][R][K][C].  One fused kernel
    (sc_multitaper_fft_f64) for the lengths it compiles; sc_taper_windows_f64 + double-precision rocFFT + transpose for
    any other window / FFT length (_stage_abc.spectra_f64)."""
    T, R, C = x.shape
    K, L = tapers_over_fs.shape
    assert L == n_window and x.dtype == torch.float64 and tapers_over_fs.dtype == torch.float64
    return _stage_abc.spectra_f64(TorchMemory(x.device), x, tapers_over_fs, T, R, C, L, n_step, n_windows, n_fft,
                                  _lib.DETREND[detrend_type], mark, use_fused)


def upload_coefficients(coef, device="cuda", f64=False):
    """Reference-layout (W,R,K,N,C) complex coefficients -> DeviceSpectra (all N bins, as given)."""
    return _stage_abc.upload_coefficients(TorchMemory(device), coef, f64)


accum_layout = _stage_abc.accum_layout


def _record_tensor(n_bins, fpb, dtype, device, row_multiple):
    """[n_bins, fpb] records; with row_multiple > 1 the allocation is rounded up to that many rows (zeroed tail) and
    the first n_bins rows are returned as a view of it -- the padded buffer (``._base``) is what a reduce-scatter over
    bins takes, without a concatenation."""
    rows = -(-n_bins // row_multiple) * row_multiple
    full = torch.empty((rows, fpb), dtype=dtype, device=device)
    if rows > n_bins:
        full[n_bins:].zero_()
    return full[:n_bins]


_PLANE_WIDTH = ((_lib.PLANE_CSM, 2), (_lib.PLANE_ABS_IM, 1), (_lib.PLANE_IM_SQ, 1), (_lib.PLANE_SIGN_IM, 1),
                (_lib.PLANE_UNIT, 2))          # record order and planes per family (sc_common.h: sc_plane_offset)


def plane_slots(planes):
    """{family bit: (first plane index, n planes)} of a record with the families ``planes``."""
    out, n = {}, 0
    for bit, width in _PLANE_WIDTH:
        if planes & bit:
            out[bit] = (n, width)
            n += width
    return out


def _channel_subset(spectra, cols):
    """The spectra of the channels ``cols`` (a LongTensor of channel indices) as a dense DeviceSpectra of its own: one gathering
    copy; an odd count gets the zero pad channel of the float32 engine."""
    X = spectra.X
    n = int(cols.numel())
    n_alloc = n if spectra.f64 else _lib.padded_channels(n, _stage_abc.MAX_KERNEL_SIGNALS)      # (n <= 256: two channel blocks)
    sub = torch.zeros(tuple(X.shape[:-1]) + (n_alloc,), dtype=X.dtype, device=X.device) if n_alloc != n else \
        torch.empty(tuple(X.shape[:-1]) + (n_alloc,), dtype=X.dtype, device=X.device)
    torch.index_select(X, X.dim() - 1, cols, out=sub[..., :n]) if n_alloc == n else sub[..., :n].copy_(X.index_select(X.dim() - 1, cols))
    assert all(st % spectra.C_alloc == 0 for st in spectra.strides), "channel subsets need spectra whose rows are dense"
    strides = tuple(st // spectra.C_alloc * n_alloc for st in spectra.strides)
    return DeviceSpectra(sub, (spectra.F, spectra.W, spectra.R, spectra.K, n), strides, spectra.n_fft, spectra.real_input, C_alloc=n_alloc)


def _accumulate_blocked(spectra, expectation_type, planes, n_freq, mark, row_multiple):
    """Stage B for MORE signals than one launch of the kernels stages (256): the reference has no limit
    (connectivity.py:447-526), a 306-channel MEG array is an ordinary input.  The channels are cut into blocks of
    _lib.BLOCK_SIGNALS; every pair of blocks (a < b) is accumulated as a request of its own on the gathered spectra of the two
    blocks (<= 256 signals: the ordinary kernels), and its 16 x 16 record tiles are copied to their places in the full record
    (_lib.tile_plan: which tiles, where to).  Every entry of the record is computed by the same kernels as for <= 256 signals;
    what the tiling costs is the tiles inside the blocks being computed once per partner (about twice the arithmetic of an
    untiled triangle at three blocks) and one gathering copy of the spectra per pair."""
    C = spectra.C
    n_bins, fpb, _, n_obs = accum_layout(spectra, expectation_type, planes, n_freq)
    NB = -(-C // 16)
    n_tiles = NB * (NB + 1) // 2
    n_planes = fpb // (n_tiles * 256)
    dtype = torch.float64 if spectra.f64 else torch.float32
    full = _record_tensor(n_bins, fpb, dtype, spectra.device, row_multiple)
    full_v = full.view(n_bins, n_planes, n_tiles, 256)
    dev = spectra.device
    for _, _, cols, src, dst in _lib.tile_plan(C):
        sub = _channel_subset(spectra, torch.as_tensor(cols, device=dev))
        rec, _ = accumulate(sub, expectation_type, planes, n_freq=n_freq, mark=mark, guard=False)    # (decided for the whole array)
        if rec.dtype != full.dtype:
            raise _lib.HipEngineError(f"a channel-block record came back as {rec.dtype}, the tiled record is {full.dtype}")
        nb_s = -(-sub.C // 16)
        rec_v = rec.view(n_bins, n_planes, nb_s * (nb_s + 1) // 2, 256)
        full_v[:, :, torch.tensor(dst, device=dev)] = rec_v[:, :, torch.tensor(src, device=dev)]
        del rec, sub
    return full, n_obs


def out_of_range(spectra, planes):
    """Does this process find the float32 request ``planes`` outside the amplitude range of the float32 kernels
    (_stage_abc.amplitude_verdict)?  What a group of processes reduces (MAX) before it calls guarded_spectra with the result."""
    return _stage_abc.amplitude_verdict(TorchMemory(spectra.device), spectra, planes) is not None


def guarded_spectra(spectra, planes, decided=None):
    """_stage_abc.amplitude_guard on this host: ``spectra``, or their complex128 copy when the request is out of range."""
    return _stage_abc.amplitude_guard(TorchMemory(spectra.device), spectra, planes, decided)


def accumulate(spectra, expectation_type, planes, n_freq=None, mark=None, use_fused=None, row_multiple=1, have=None,
               fold=True, ws_owner=None, guard=True):
    """Stage B: un-normalised accumulator record tensor [n_bins, floats_per_bin] (float32; float64 records from
    complex128 spectra) -- one call of _stage_abc.accumulate; what is tensor arithmetic of this host happens around it.
    ``row_multiple``: see _record_tensor (trial-sharded callers pass the world size).
    ``fold=False`` (planes-format path only; ignored elsewhere): when stage B split every bin over several workgroups, their
    partial records are NOT summed -- the result is then ONE 3-D tensor [n_parts, n_bins, floats_per_bin] of its own (the sum
    over axis 0, in part order, is the record): measure() / measure_multi() add the parts while their kernel reads them (one pass
    and one record round trip less), fold_parts() gives the 2-D record to any other consumer.
    ``have`` = (planes_old, record_old), float64 engine only: families already accumulated for the same spectra and
    expectation are copied over (a strided device copy) and only the missing ones are computed -- its CSM and
    per-observation planes are separate kernels, so a wPLI after a coherence costs the |Im s| plane alone.
    ``ws_owner``: see _workspace (a dict that owns the split-bin scratch of this call instead of the per-device cache).
    ``guard``: a float32 request whose (Im s)^2 or s / |s| would leave the float32 range is accumulated from a complex128 copy
    of the spectra and comes back as a float64 record, padded rows and channel-block tiling included (_stage_abc.amplitude_guard:
    one reduction over the spectra and one small read-back per spectra object, for requests with these families only).  False:
    the caller has decided already -- trial-sharded callers decide once for their group (parallel.group_guarded_spectra), the
    tiling for the whole array; a captured pass cannot read back and is not guarded either (``ws_owner``)."""
    if guard and ws_owner is None:
        spectra = guarded_spectra(spectra, planes)
    if spectra.C > _stage_abc.MAX_KERNEL_SIGNALS:
        # planes-format spectra go straight to sc_fused2.hip, which plans its launches over any number of 32-channel blocks (round 6);
        # every other request beyond 256 signals is tiled over channel-block pairs
        direct = (not spectra.f64 and spectra.P is not None and use_fused is not False
                  and _stage_abc.fused2_takes(spectra.desc(expectation_type, n_freq, padded=True), planes))
        if not direct:
            return _accumulate_blocked(spectra, expectation_type, planes, n_freq, mark, row_multiple)
    out = which = None
    copy_have = spectra.f64 and have is not None
    if row_multiple != 1 or copy_have:
        # the record is this host's to shape: padded rows for a reduce-scatter, or partly filled from a record at hand
        n_bins, fpb, _, _ = accum_layout(spectra, expectation_type, planes, n_freq)
        out = _record_tensor(n_bins, fpb, torch.float64 if spectra.f64 else torch.float32, spectra.device, row_multiple)
        if copy_have and have[1].dtype == torch.float64 and have[1].shape[0] == n_bins and (have[0] & planes):
            which = planes
            old_planes, old = have
            new_slots, old_slots = plane_slots(planes), plane_slots(old_planes)
            n_new, n_old = sum(w for _, w in new_slots.values()), sum(w for _, w in old_slots.values())
            new_v, old_v = out.view(n_bins, n_new, fpb // n_new), old.view(n_bins, n_old, old.shape[1] // n_old)
            for bit, (i_new, width) in new_slots.items():
                if bit in old_slots:
                    new_v[:, i_new:i_new + width].copy_(old_v[:, old_slots[bit][0]:old_slots[bit][0] + width])
                    which &= ~bit
    accum, n_obs = _stage_abc.accumulate(TorchMemory(spectra.device), spectra, expectation_type, planes, n_freq, which, out, fold,
                                         ws_owner, use_fused, mark)
    if accum.dim() == 3 and accum.shape[0] == 1:
        accum = accum[0]                                   # (the kernel did not split the bins: an ordinary record)
    return accum, n_obs


def fold_parts(accum):
    """[n_parts, n_bins, floats_per_bin] partial records -> their sum in part order (the record a folding pass of stage B
    would have written, bit for bit: the same additions in the same order); a 2-D record is returned as it is.  The folded
    record is kept on the tensor, so several consumers pay for one fold."""
    if accum.dim() != 3:
        return accum
    cached = getattr(accum, "_sc_folded", None)
    if cached is None:
        cached = accum[0].clone()
        for k in range(1, accum.shape[0]):
            cached.add_(accum[k])
        accum._sc_folded = cached
    return cached


def _record_and_parts(accum, summed_by_kernel=True):
    """(2-D record, partial records or None): contiguous partial records [n_parts > 1, n_bins, floats_per_bin] go to the epilogue as
    they are when its kernel sums them in part order while it reads (``summed_by_kernel``); they are folded here otherwise."""
    if accum.dim() != 3:
        return accum, None
    if summed_by_kernel and accum.shape[0] > 1 and accum.is_contiguous():
        return accum[0], accum
    return fold_parts(accum), None                       # part (= rank) order


def measure(accum, n_signals, planes, n_obs, which, out=None, wide=None):
    """Stage C: one measure from an accumulator tensor (after any cross-GPU sum; partial records: sc_measure_parts, every measure,
    power and the complex-valued ones included).  ``wide``: write float64 / complex128 (what the reference returns) straight from
    the epilogue; default: wide for double records."""
    accum, parts = _record_and_parts(accum)
    if wide is None:
        wide = accum.dtype == torch.float64
    return _stage_abc.measure(TorchMemory(accum.device), accum, n_signals, planes, n_obs, which, wide, parts, out)


def measure_multi(accum, n_signals, planes, n_obs, which, wide=None, stacked=False):
    """Stage C for several real-valued C x C measures of one record: ONE launch reads the record once
    (sc_measure_multi_*); complex measures / power, or more than four, go through measure().
    ``stacked``: the results are the slices of ONE [n_measures, n_bins, C, C] tensor (returned as ``outs[0]._base``'s
    views) when the one-launch form applies -- the trial-sharded path then gathers all measures in one collective.
    ``accum`` may be 3-D, [n_parts, n_bins, floats_per_bin]: partial records (the blocks received from the other ranks)
    that the epilogue sums in part order while it reads them (sc_measure_multi_parts) -- or, where the one-launch form
    does not apply, that are summed first."""
    which = list(which)
    accum, parts = _record_and_parts(accum, _stage_abc.one_launch(which, True))
    if wide is None:
        wide = accum.dtype == torch.float64
    outs = None
    if stacked and _stage_abc.one_launch(which, parts is not None):
        block = torch.empty((len(which), accum.shape[0], n_signals, n_signals), dtype=torch.float64 if wide else torch.float32,
                            device=accum.device)
        outs = list(block.unbind(0))
    return _stage_abc.measure_multi(TorchMemory(accum.device), accum, n_signals, planes, n_obs, which, wide, parts, outs)


# ---- stage D: the call sequences live in _stage_d.py (shared with the torch-free host); here are the memory adapter of this host
# and the public functions, each one call into its driver ---------------------------------------------------------------------
MAX_WILSON_ITERATIONS = _stage_d.MAX_WILSON_ITERATIONS
check_max_iterations = _stage_d.check_max_iterations
GRANGER_WORK_BYTES = _lib.GRANGER_WORK_BYTES      # (the bound the drivers read is _lib.GRANGER_WORK_BYTES)


def granger_pairwise(accum, n_groups, n_freq_accum, n_fft, n_signals, planes, n_obs, pairs,
                     tolerance=1e-8, max_iterations=60):
    """Batched 2x2 Wilson + spectral Granger (sc_wilson.hip): _stage_d.granger_pairwise on device tensors.  Returns (out, n_iter,
    status, summary), n_iter / status [n_groups, n_pairs] flattened."""
    return _stage_d.granger_pairwise(TorchMemory(accum.device), accum, n_groups, n_freq_accum, n_fft, n_signals, planes, n_obs, pairs,
                                     tolerance, max_iterations)


def mvar_factor(n_groups, n_fft, n_signals, accum=None, n_freq_accum=0, planes=0, n_obs=1, spectra=None,
                tolerance=1e-8, max_iterations=60):
    """Full C x C Wilson factor (sc_mvar.hip) of accumulator records or of a two-sided complex128 spectrum
    tensor [n_groups, n_fft, C, C].  Returns (G [n_groups, n_fft, C, C] complex128, n_iter, status, summary)."""
    src = accum if accum is not None else spectra
    return _stage_d.mvar_factor(TorchMemory(src.device), n_groups, n_fft, n_signals, accum, n_freq_accum, planes, n_obs, spectra,
                                tolerance, max_iterations)


def conditional_granger(G, n_groups, n_fft, n_signals, accum=None, n_freq_accum=0, planes=0, n_obs=1, spectra=None,
                        tolerance=1e-8, max_iterations=60):
    """Conditional spectral Granger prediction (sc_conditional.hip) from the cached full factor ``G``: _stage_d.conditional_granger.
    Returns (out [n_groups, n_fft/2+1, C, C] float64, n_iter [C, n_groups], status [C, n_groups], summary)."""
    return _stage_d.conditional_granger(TorchMemory(G.device), G, n_groups, n_fft, n_signals, accum, n_freq_accum, planes, n_obs,
                                        spectra, tolerance, max_iterations)


def blockwise_granger(n_groups, n_fft, n_signals, batches, n_blocks, accum=None, n_freq_accum=0, planes=0, n_obs=1, spectra=None,
                       tolerance=1e-8, max_iterations=60, device=None):
    """Blockwise spectral Granger prediction (sc_blockwise.hip): _stage_d.blockwise_granger.  Returns (out [n_groups, n_fft/2+1,
    n_blocks, n_blocks] float64, n_iter [pairs, n_groups], status [pairs, n_groups] in the order of ``batches``, summary)."""
    dev = device if device is not None else (accum if accum is not None else spectra).device
    return _stage_d.blockwise_granger(TorchMemory(dev), n_groups, n_fft, n_signals, batches, n_blocks, accum, n_freq_accum, planes,
                                      n_obs, spectra, tolerance, max_iterations)


def mvar_measure(G, which):
    """A directed MVAR measure / model quantity (``_lib.MVAR_*``) from the minimum-phase factor G."""
    return _stage_d.mvar_measure(TorchMemory(G.device), G, which)


def global_coherence(accum, n_groups, n_freq_accum, n_fft, n_signals, planes, n_obs, max_rank, ascending):
    """Leading eigenpairs of the CSM per (window, two-sided bin) (sc_global.hip)."""
    return _stage_d.global_coherence(TorchMemory(accum.device), accum, n_groups, n_freq_accum, n_fft, n_signals, planes, n_obs,
                                     max_rank, ascending)


def canonical_coherence(accum, n_signals, planes, n_obs, groups):
    """groups: list of int arrays (channel indices per group).  Returns ([n_bins, G, G] float64, n_fail)."""
    return _stage_d.canonical_coherence(TorchMemory(accum.device), accum, n_signals, planes, n_obs, groups)


def imaginary_interaction(accum, n_signals, planes, n_obs, members, sizes):
    """members / sizes: _lib.member_table of the groups.  Returns (MIC, MIM [n_bins, G, G] float64, n_fail)."""
    return _stage_d.imaginary_interaction(TorchMemory(accum.device), accum, n_signals, planes, n_obs, members, sizes)


def imaginary_interaction_vectors(accum, n_signals, planes, n_obs, members, sizes):
    """members / sizes: _lib.member_table of the groups.  Returns (MIC [n_bins, G, G], filters, patterns [n_bins, G, G, max group
    size] float64, n_fail)."""
    return _stage_d.imaginary_interaction_vectors(TorchMemory(accum.device), accum, n_signals, planes, n_obs, members, sizes)


def canonical_coherence_vectors(accum, n_signals, planes, n_obs, members, sizes):
    """members / sizes: _lib.member_table of the groups.  Returns (coherence [n_bins, G, G], coherences [n_bins, G, G, max group
    size], filters, patterns [n_bins, G, G, max group size, 2] (re, im) float64, n_fail)."""
    return _stage_d.canonical_coherence_vectors(TorchMemory(accum.device), accum, n_signals, planes, n_obs, members, sizes)


def linear_dependence(accum, n_signals, planes, n_obs, members, sizes, want):
    """Total, instantaneous and lagged linear dependence between the groups (sc_dependence.hip): _stage_d.linear_dependence.
    Returns ({name: [n_bins, G, G] float64 tensor} for the names in ``want``, n_fail)."""
    return _stage_d.linear_dependence(TorchMemory(accum.device), accum, n_signals, planes, n_obs, members, sizes, want)


def partial_coherence(accum, n_signals, planes, n_obs, want):
    """Partial and multiple coherence of every bin record (sc_partial.hip): _stage_d.partial_coherence.  Returns ({name: tensor}
    for the names of ``want`` out of "coherency", "magnitude", "multiple", n_fail)."""
    return _stage_d.partial_coherence(TorchMemory(accum.device), accum, n_signals, planes, n_obs, want)


def partial_coherence_given(accum, n_signals, planes, n_obs, kept, given, want):
    """Partial and multiple coherence of the signals ``kept`` given the signals ``given`` (sc_partial.hip):
    _stage_d.partial_coherence_given.  Returns ({name: tensor} for the names in ``want``, (n_failed, n_explained))."""
    return _stage_d.partial_coherence_given(TorchMemory(accum.device), accum, n_signals, planes, n_obs, kept, given, want)


def jackknife(spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq=None, unit_range=None):
    """Delete-one jackknife sums (sc_jackknife.hip) of the spectra against the total CSM record ``total`` (partial records are
    folded first): _stage_d.jackknife.  Returns (float64 device tensor laid out as _lib.jackknife_blocks says, n_bins)."""
    return _stage_d.jackknife(TorchMemory(spectra.device), spectra, expectation_type, fold_parts(total), planes, measures, over,
                              n_units_total, n_freq, unit_range)


def jackknife_phase(spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq=None, unit_range=None):
    """Delete-one jackknife sums of the phase-lag family (jk_phase_kernel of sc_jackknife.hip) against the total accumulator record
    ``total`` with the families ``planes`` (partial records are folded first): _stage_d.jackknife_phase."""
    return _stage_d.jackknife_phase(TorchMemory(spectra.device), spectra, expectation_type, fold_parts(total), planes, measures,
                                    over, n_units_total, n_freq, unit_range)


def jackknife_phase_totals(spectra, expectation_type, planes, over, n_freq=None, unit_range=None):
    """The float64 total record of jackknife_phase from the spectra themselves: _stage_d.jackknife_phase_totals."""
    return _stage_d.jackknife_phase_totals(TorchMemory(spectra.device), spectra, expectation_type, planes, over, n_freq, unit_range)


def seed_jackknife_totals(spectra, expectation_type, seeds, targets, planes, over, n_freq=None, unit_range=None):
    """The float64 total seed record of seed_jackknife from the spectra themselves: _stage_d.seed_jackknife_totals."""
    return _stage_d.seed_jackknife_totals(TorchMemory(spectra.device), spectra, expectation_type, seeds, targets, planes, over, n_freq,
                                          unit_range)


def seed_jackknife(spectra, expectation_type, seeds, targets, total, planes, measures, over, n_units_total, n_freq=None,
                   unit_range=None):
    """Delete-one jackknife sums of ``seeds`` against ``targets`` (sc_seed_jackknife.hip) against the total seed record ``total`` with
    the families ``planes``: _stage_d.seed_jackknife."""
    return _stage_d.seed_jackknife(TorchMemory(spectra.device), spectra, expectation_type, seeds, targets, total, planes, measures,
                                   over, n_units_total, n_freq, unit_range)


class GraphedMeasures:
    """Stage A, stage B and the epilogue of ONE fixed request, captured once in a hipGraph and replayed per time series.

    A small request -- BASELINE configs[1]: 32 channels x 100 trials x 1024 samples, 82 us of kernels in three launches -- is bound
    by the host: every launch costs the CPU 5-10 us, and the eager pass takes 0.11 ms for 0.08 ms of device work.  Captured once
    (the kernels, their arguments, the buffers they run on), the pass replays with ONE launch; the results are bit-identical to
    the eager pass (tests/test_gpu_configs.py::test_graphed_measures_replay_equals_the_eager_pass).  This is for callers that
    evaluate the same geometry over and over (a sliding analysis of a stream, a parameter scan over data sets of one shape): the
    input and the results live in buffers the object owns.

        g = engine.GraphedMeasures((T, R, C), tapers_over_fs, n_window, n_step, n_fft, "constant", "trials_tapers",
                                   [_lib.M_COHERENCY])
        out, = g(x)          # x: (T, R, C) float32 tensor (device, or host: copied in); out is overwritten by the next call

    float32 engine, complex64 spectra (the planes format starts at 256 MB of spectra, far above what a graph helps with).
    """

    def __init__(self, shape, tapers_over_fs, n_window, n_step, n_fft, detrend_type, expectation_type, measures, device=None):
        T, R, C = (int(v) for v in shape)
        dev = tapers_over_fs.device if device is None else torch.device(device)
        self.x = torch.zeros((T, R, C), dtype=torch.float32, device=dev)
        self.measures = list(measures)
        self.planes = 0
        for w in self.measures:
            self.planes |= _lib.MEASURE_PLANES[w]
        n_windows = int(np.floor(T / n_step - n_window / n_step + 1))
        h = tapers_over_fs.to(dev)
        self._ws = {}                                 # the split-bin scratch of the captured stage B: this object's own

        def run():
            sp = multitaper_spectra(self.x, h, n_window, n_step, n_fft, n_windows, detrend_type)
            accum, n_obs = accumulate(sp, expectation_type, self.planes, ws_owner=self._ws)
            return measure_multi(accum, C, self.planes, n_obs, self.measures)

        self._eager = run
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                 # twiddles, function attributes, the allocator's blocks: outside the capture
            run()
            run()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = run()

    def __call__(self, x=None):
        if x is not None:
            self.x.copy_(torch.as_tensor(x), non_blocking=True)
        self.graph.replay()
        return self.out

    def eager(self, x=None):
        """The same pass launch by launch (for comparison)."""
        if x is not None:
            self.x.copy_(torch.as_tensor(x), non_blocking=True)
        return self._eager()
