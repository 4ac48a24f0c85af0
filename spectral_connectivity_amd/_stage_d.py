"""Stage D: the call sequences of every measure that runs on accumulated cross-spectral records, written once for both hosts.

Each function drives one entry-point family of include/sc_hip.h -- sizes the workspace, cuts the job into chunks under the
workspace bound (``_lib.GRANGER_WORK_BYTES`` / ``_lib.CONDITIONAL_WORK_BYTES``, read at call time), keeps the output on every
call but the first, offsets the per-chunk pointers and combines the three-int summaries -- and never imports torch.  What differs
between the hosts is behind the memory adapter ``mem``, the first argument (engine.TorchMemory: tensors on the current stream;
numpy_host.NumpyMemory: DeviceArray over the library's own allocator):

    mem.empty(shape, dtype) / mem.zeros(shape, dtype)    a device array (NumPy dtypes: uint8, int32, float64, complex128)
    mem.upload(numpy_array)                              a device array holding a copy
    mem.ptr(array, first_row=0)                          c_void_p of the array's row ``first_row``
    mem.stream()                                         the stream every call is launched on
    mem.is_f64(record)                                   records of doubles (the SC_RECORD_F64 bit of ``planes``)
    mem.fill_nan(array)                                  NaN into an output no call wrote
    mem.read_int(array)                                  the first int32 of an array, on the host
    mem.hstack(chunks, n_rows)                           flat [n_rows, n_0], [n_rows, n_1], ... joined along the columns, flat
    mem.download(array)                                  NumPy copy (the callers' side: no driver downloads a result)

Returned arrays are device arrays of the host's own type.  A new stage-D measure adds its entry point to ``_lib.SYMBOLS``, one
driver here and one thin wrapper in engine.py.
"""
import ctypes
from ctypes import byref, c_int64

import numpy as np

from . import _lib

MAX_WILSON_ITERATIONS = 1024      # iterations the device kernels can log (WILSON_HIST in csrc/sc_wilson_loop.h)


def check_max_iterations(max_iterations):
    """The reference takes any positive count (minimum_phase_decomposition.py:227-322); the device kernels log at most 1024."""
    if not 1 <= int(max_iterations) <= MAX_WILSON_ITERATIONS:
        raise ValueError(f"max_iterations must be between 1 and {MAX_WILSON_ITERATIONS} on the device path (got {max_iterations}); "
                         "Wilson's iteration converges in tens of steps or not at all")
    return int(max_iterations)


def _planes(mem, accum, planes):
    """`planes` as the consumers of the records ``accum`` want it (a spectrum tensor instead of records: as given)."""
    return planes if accum is None else _lib.record_planes(planes, mem.is_f64(accum))


def _ptr(mem, array):
    return None if array is None else mem.ptr(array)


def _size(fn, what, *args):
    """A workspace query of the library: its byte count."""
    nbytes = ctypes.c_size_t()
    _lib.check(fn(*args, byref(nbytes)), what)
    return nbytes.value


def _wilson(mem, fn, what, total, *args):
    """One call of a Wilson entry point (its last two arguments are the summary and the stream); its summary = (iterations run,
    problems not converged, identity starts) goes into ``total`` as max, sum, sum."""
    summary = (ctypes.c_int32 * 3)(0, 0, 0)
    _lib.check(fn(*args, summary, mem.stream()), what)
    total[0] = max(total[0], summary[0])
    total[1] += summary[1]
    total[2] += summary[2]


def granger_workspace(mem, n_groups, n_problems, n_fft):
    """(workspace, its bytes) of the 2x2 Wilson kernels for ``n_problems`` problems per group (sc_granger_pairwise_f64,
    sc_wilson_factor_f64)."""
    nbytes = _size(_lib._handle().sc_granger_workspace_bytes, "sc_granger_workspace_bytes", n_groups, n_problems, n_fft)
    return mem.empty((nbytes,), np.uint8), nbytes


def granger_pairwise(mem, accum, n_groups, n_freq_accum, n_fft, n_signals, planes, n_obs, pairs, tolerance=1e-8, max_iterations=60):
    """Batched 2x2 Wilson + spectral Granger (sc_wilson.hip).  Returns (out [n_groups, n_fft/2+1, C, C] float64, n_iter, status,
    summary): n_iter / status are [n_groups, n_pairs] flattened, whatever the chunking, and summary = (iterations run, problems not
    converged, problems started from the identity because their lag-0 covariance was not positive definite).  A long pair list is
    walked in chunks that bound the workspace (160 bytes per problem and bin); every chunk writes its pairs into the same output."""
    lib = _lib._handle()
    max_iterations = check_max_iterations(max_iterations)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = pairs.shape[0]
    out = mem.empty((n_groups, n_fft // 2 + 1, n_signals, n_signals), np.float64)
    chunk = int(max(1, min(n_pairs, _lib.GRANGER_WORK_BYTES // (n_groups * n_fft * 160))))
    work, nbytes = granger_workspace(mem, n_groups, chunk, n_fft)
    d_pairs = mem.upload(pairs)
    total, n_iter, status = [0, 0, 0], [], []
    for p0 in range(0, n_pairs, chunk):
        n = min(chunk, n_pairs - p0)
        n_iter.append(mem.empty((n_groups * n,), np.int32))          # [n_groups, n] of this chunk
        status.append(mem.empty((n_groups * n,), np.int32))
        _wilson(mem, lib.sc_granger_pairwise_f64, "sc_granger_pairwise_f64", total,
                mem.ptr(accum), n_groups, n_freq_accum, n_fft, n_signals, _planes(mem, accum, planes), n_obs, mem.ptr(d_pairs, p0), n,
                tolerance, max_iterations, mem.ptr(work), nbytes, _lib.GRANGER_KEEP_OUTPUT if p0 else 0, mem.ptr(out),
                mem.ptr(n_iter[-1]), mem.ptr(status[-1]))
    return out, mem.hstack(n_iter, n_groups), mem.hstack(status, n_groups), tuple(total)


def _mvar_workspace(mem, n_groups, n_signals, n_fft):
    nbytes = _size(_lib._handle().sc_mvar_workspace_bytes, "sc_mvar_workspace_bytes", n_groups, n_signals, n_fft)
    return mem.empty((nbytes,), np.uint8), nbytes


def mvar_factor(mem, n_groups, n_fft, n_signals, accum=None, n_freq_accum=0, planes=0, n_obs=1, spectra=None, tolerance=1e-8,
                max_iterations=60):
    """Full C x C Wilson factor (sc_mvar.hip) of accumulator records or of a two-sided complex128 spectrum array
    [n_groups, n_fft, C, C].  Returns (G [n_groups, n_fft, C, C] complex128, n_iter, status, summary)."""
    max_iterations = check_max_iterations(max_iterations)
    work, nbytes = _mvar_workspace(mem, n_groups, n_signals, n_fft)
    G = mem.empty((n_groups, n_fft, n_signals, n_signals), np.complex128)
    n_iter, status = mem.empty((n_groups,), np.int32), mem.empty((n_groups,), np.int32)
    total = [0, 0, 0]
    _wilson(mem, _lib._handle().sc_mvar_factor_f64, "sc_mvar_factor_f64", total,
            _ptr(mem, accum), _ptr(mem, spectra), n_groups, n_freq_accum, n_fft, n_signals, _planes(mem, accum, planes), n_obs,
            tolerance, max_iterations, mem.ptr(work), nbytes, mem.ptr(G), mem.ptr(n_iter), mem.ptr(status))
    return G, n_iter, status, tuple(total)


def mvar_measure(mem, G, which):
    """A directed MVAR measure / model quantity (``_lib.MVAR_*``) from the minimum-phase factor G."""
    n_groups, n_fft, C, _ = G.shape
    F = n_fft // 2 + 1
    work, nbytes = _mvar_workspace(mem, n_groups, C, n_fft)
    if which == _lib.MVAR_NOISE_COVARIANCE:
        out = mem.empty((n_groups, C, C), np.float64)
    else:
        out = mem.empty((n_groups, F, C, C), np.complex128 if which in (_lib.MVAR_TRANSFER, _lib.MVAR_COEFFICIENTS) else np.float64)
    _lib.check(_lib._handle().sc_mvar_measure_f64(mem.ptr(G), n_groups, n_fft, C, which, mem.ptr(out), mem.ptr(work), nbytes,
                                                  mem.stream()), "sc_mvar_measure_f64")
    return out


def conditional_granger(mem, G, n_groups, n_fft, n_signals, accum=None, n_freq_accum=0, planes=0, n_obs=1, spectra=None,
                        tolerance=1e-8, max_iterations=60):
    """Conditional spectral Granger prediction (sc_conditional.hip) from the cached full factor ``G`` [n_groups, n_fft, C, C]
    and the records (or a two-sided complex128 spectrum array) it was factored from: one reduced (C - 1)-signal Wilson
    factorisation per dropped signal, batched over the dropped signals of a chunk.  Returns (out [n_groups, n_fft/2+1, C, C]
    float64, out[..., i, j] = j -> i given the rest, n_iter [C, n_groups], status [C, n_groups], summary) with summary =
    (iterations run, reduced problems not converged, identity starts)."""
    lib = _lib._handle()
    max_iterations = check_max_iterations(max_iterations)
    C = n_signals

    def ws(n_dropped):
        return _size(lib.sc_conditional_granger_workspace_bytes, "sc_conditional_granger_workspace_bytes", n_groups, C, n_fft,
                     n_dropped)

    chunk = _lib.conditional_chunk(n_groups, C, ws)
    nbytes = ws(chunk)
    work = mem.empty((nbytes,), np.uint8)
    out = mem.empty((n_groups, n_fft // 2 + 1, C, C), np.float64)
    n_iter, status = mem.empty((C, n_groups), np.int32), mem.empty((C, n_groups), np.int32)
    dropped = mem.upload(np.arange(C, dtype=np.int32))
    total = [0, 0, 0]
    for j0 in range(0, C, chunk):
        _wilson(mem, lib.sc_conditional_granger_f64, "sc_conditional_granger_f64", total,
                _ptr(mem, accum), _ptr(mem, spectra), n_groups, n_freq_accum, n_fft, C, _planes(mem, accum, planes), n_obs, mem.ptr(G),
                mem.ptr(dropped, j0), min(chunk, C - j0), tolerance, max_iterations, mem.ptr(work), nbytes,
                _lib.CONDITIONAL_KEEP_OUTPUT if j0 else 0, mem.ptr(out), mem.ptr(n_iter, j0), mem.ptr(status, j0))
    return out, n_iter, status, tuple(total)


def blockwise_granger(mem, n_groups, n_fft, n_signals, batches, n_blocks, accum=None, n_freq_accum=0, planes=0, n_obs=1, spectra=None,
                      tolerance=1e-8, max_iterations=60):
    """Blockwise spectral Granger prediction (sc_blockwise.hip) from the records (or a two-sided complex128 spectrum array):
    one m-signal Wilson factorisation per (block pair, group), the pairs of one size m batched under the workspace cap.
    ``batches``: {m: (members [n, m], split [n], cell [n, 2])} int32 arrays (_lib.blockwise_batches).  Returns (out [n_groups,
    n_fft/2+1, n_blocks, n_blocks] float64, out[..., a, b] = b -> a, NaN where no pair was computed, n_iter [pairs, n_groups],
    status [pairs, n_groups] in the order of the batches, summary) with summary = (iterations run, problems not converged,
    identity starts)."""
    lib = _lib._handle()
    max_iterations = check_max_iterations(max_iterations)
    n_total = sum(len(split) for _, split, _ in batches.values())
    out = mem.empty((n_groups, n_fft // 2 + 1, n_blocks, n_blocks), np.float64)
    n_iter, status = mem.zeros((n_total, n_groups), np.int32), mem.zeros((n_total, n_groups), np.int32)
    total = [0, 0, 0]
    row, flags = 0, 0              # the first call NaN-fills the output, the others keep it
    for m, (members, split, cell) in batches.items():
        n_pairs = len(split)

        def ws(n, m=m):
            return _size(lib.sc_blockwise_granger_workspace_bytes, "sc_blockwise_granger_workspace_bytes", n_groups, m, n_fft, n)

        chunk = _lib.blockwise_chunk(n_groups, n_pairs, ws)
        nbytes = ws(chunk)
        work = mem.empty((nbytes,), np.uint8)
        d_members, d_split, d_cell = mem.upload(members), mem.upload(split), mem.upload(cell)
        for q0 in range(0, n_pairs, chunk):
            _wilson(mem, lib.sc_blockwise_granger_f64, "sc_blockwise_granger_f64", total,
                    _ptr(mem, accum), _ptr(mem, spectra), n_groups, n_freq_accum, n_fft, n_signals, _planes(mem, accum, planes), n_obs,
                    mem.ptr(d_members, q0), mem.ptr(d_split, q0), mem.ptr(d_cell, q0), min(chunk, n_pairs - q0), m, n_blocks,
                    tolerance, max_iterations, mem.ptr(work), nbytes, flags, mem.ptr(out), mem.ptr(n_iter, row + q0),
                    mem.ptr(status, row + q0))
            flags = _lib.BLOCKWISE_KEEP_OUTPUT
        row += n_pairs
    if not flags:
        mem.fill_nan(out)
    return out, n_iter, status, tuple(total)


def global_coherence(mem, accum, n_groups, n_freq_accum, n_fft, n_signals, planes, n_obs, max_rank, ascending):
    """Leading eigenpairs of the CSM per (window, two-sided bin) (sc_global.hip): (values [n_groups, n_fft, max_rank] float64,
    vectors [n_groups, n_fft, C, max_rank] complex128)."""
    values = mem.empty((n_groups, n_fft, max_rank), np.float64)
    vectors = mem.empty((n_groups, n_fft, n_signals, max_rank), np.complex128)
    _lib.check(_lib._handle().sc_global_coherence_f64(mem.ptr(accum), n_groups, n_freq_accum, n_fft, n_signals,
                                                      _planes(mem, accum, planes), n_obs, max_rank, int(ascending), mem.ptr(values),
                                                      mem.ptr(vectors), mem.stream()), "sc_global_coherence_f64")
    return values, vectors


def canonical_coherence(mem, accum, n_signals, planes, n_obs, groups):
    """groups: list of int arrays (channel indices per group).  Returns ([n_bins, G, G] float64, n_fail)."""
    members, sizes, _ = _lib.member_table(groups)
    G, n_bins = len(sizes), accum.shape[0]
    d_members, d_sizes = mem.upload(members), mem.upload(sizes)
    out = mem.empty((n_bins, G, G), np.float64)
    fail = mem.zeros((1,), np.int32)
    _lib.check(_lib._handle().sc_canonical_coherence_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes), n_obs,
                                                         mem.ptr(d_members), mem.ptr(d_sizes), G, int(sizes.max()), mem.ptr(out),
                                                         mem.ptr(fail), mem.stream()), "sc_canonical_coherence_f64")
    return out, mem.read_int(fail)


def imaginary_interaction(mem, accum, n_signals, planes, n_obs, members, sizes):
    """members / sizes: _lib.member_table of the groups.  Returns (MIC, MIM [n_bins, G, G] float64, n_fail)."""
    G, n_bins = len(sizes), accum.shape[0]
    d_members, d_sizes = mem.upload(members), mem.upload(sizes)
    mic, mim = mem.empty((n_bins, G, G), np.float64), mem.empty((n_bins, G, G), np.float64)
    fail = mem.zeros((1,), np.int32)
    _lib.check(_lib._handle().sc_imaginary_interaction_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes), n_obs,
                                                           mem.ptr(d_members), mem.ptr(d_sizes), G, int(sizes.max()), mem.ptr(mic),
                                                           mem.ptr(mim), mem.ptr(fail), mem.stream()), "sc_imaginary_interaction_f64")
    return mic, mim, mem.read_int(fail)


def imaginary_interaction_vectors(mem, accum, n_signals, planes, n_obs, members, sizes):
    """The vectors that attain MIC (sc_imaginary_interaction_vectors_f64).  members / sizes: _lib.member_table of the groups.
    Returns (MIC [n_bins, G, G], filters, patterns [n_bins, G, G, max group size] float64, n_fail)."""
    G, n_bins, n_max = len(sizes), accum.shape[0], int(sizes.max())
    d_members, d_sizes = mem.upload(members), mem.upload(sizes)
    mic = mem.empty((n_bins, G, G), np.float64)
    filters, patterns = mem.empty((n_bins, G, G, n_max), np.float64), mem.empty((n_bins, G, G, n_max), np.float64)
    fail = mem.zeros((1,), np.int32)
    _lib.check(_lib._handle().sc_imaginary_interaction_vectors_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes),
                                                                   n_obs, mem.ptr(d_members), mem.ptr(d_sizes), G, n_max,
                                                                   mem.ptr(mic), mem.ptr(filters), mem.ptr(patterns), mem.ptr(fail),
                                                                   mem.stream()), "sc_imaginary_interaction_vectors_f64")
    return mic, filters, patterns, mem.read_int(fail)


def canonical_coherence_vectors(mem, accum, n_signals, planes, n_obs, members, sizes):
    """The vectors that attain canonical coherence and every canonical coherence (sc_canonical_coherence_vectors_f64).
    members / sizes: _lib.member_table of the groups.  Returns (coherence [n_bins, G, G], coherences [n_bins, G, G, n_max],
    filters, patterns [n_bins, G, G, n_max, 2] (re, im), all float64, n_fail)."""
    G, n_bins, n_max = len(sizes), accum.shape[0], int(sizes.max())
    d_members, d_sizes = mem.upload(members), mem.upload(sizes)
    coherence, coherences = mem.empty((n_bins, G, G), np.float64), mem.empty((n_bins, G, G, n_max), np.float64)
    filters, patterns = mem.empty((n_bins, G, G, n_max, 2), np.float64), mem.empty((n_bins, G, G, n_max, 2), np.float64)
    fail = mem.zeros((1,), np.int32)
    _lib.check(_lib._handle().sc_canonical_coherence_vectors_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes),
                                                                 n_obs, mem.ptr(d_members), mem.ptr(d_sizes), G, n_max,
                                                                 mem.ptr(coherence), mem.ptr(coherences), mem.ptr(filters),
                                                                 mem.ptr(patterns), mem.ptr(fail), mem.stream()),
               "sc_canonical_coherence_vectors_f64")
    return coherence, coherences, filters, patterns, mem.read_int(fail)


def linear_dependence(mem, accum, n_signals, planes, n_obs, members, sizes, want):
    """Total, instantaneous and lagged linear dependence between the groups (sc_dependence.hip).  members / sizes:
    _lib.member_table of the groups; ``want``: names out of "total", "instantaneous", "lagged" -- one call serves them all.
    Returns ({name: [n_bins, G, G] float64 device array}, n_fail)."""
    G, n_bins = len(sizes), accum.shape[0]
    d_members, d_sizes = mem.upload(members), mem.upload(sizes)
    out = {name: mem.empty((n_bins, G, G), np.float64) for name in want}
    fail = mem.zeros((1,), np.int32)
    _lib.check(_lib._handle().sc_linear_dependence_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes), n_obs,
                                                       mem.ptr(d_members), mem.ptr(d_sizes), G, int(sizes.max()),
                                                       _ptr(mem, out.get("total")), _ptr(mem, out.get("instantaneous")),
                                                       _ptr(mem, out.get("lagged")), mem.ptr(fail), mem.stream()),
               "sc_linear_dependence_f64")
    return out, mem.read_int(fail)


def partial_coherence(mem, accum, n_signals, planes, n_obs, want):
    """Partial and multiple coherence of every bin record (sc_partial.hip).  ``want``: names out of "coherency", "magnitude",
    "multiple" -- one call serves them all.  Returns ({name: device array}, n_fail): coherency complex128 and magnitude float64
    [n_bins, C, C], multiple float64 [n_bins, C]."""
    n_bins = accum.shape[0]
    shapes = {"coherency": ((n_bins, n_signals, n_signals), np.complex128), "magnitude": ((n_bins, n_signals, n_signals), np.float64),
              "multiple": ((n_bins, n_signals), np.float64)}
    out = {name: mem.empty(*shapes[name]) for name in want}
    fail = mem.zeros((1,), np.int32)
    _lib.check(_lib._handle().sc_partial_coherence_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes), n_obs,
                                                       _ptr(mem, out.get("coherency")), _ptr(mem, out.get("magnitude")),
                                                       _ptr(mem, out.get("multiple")), mem.ptr(fail), mem.stream()),
               "sc_partial_coherence_f64")
    return out, mem.read_int(fail)


def partial_coherence_given(mem, accum, n_signals, planes, n_obs, kept, given, want):
    """Partial and multiple coherence given a chosen set (sc_partial_coherence_given_f64) of every bin record.  ``kept`` / ``given``:
    the int32 arrays of _lib.partial_given_indices; ``want`` as partial_coherence.  Returns ({name: device array}, (records that
    failed, (record, kept signal) cases without a residual)): coherency complex128 and magnitude float64 [n_bins, a, a] in the order
    of ``kept``, multiple float64 [n_bins, a]."""
    n_bins, a = accum.shape[0], len(kept)
    shapes = {"coherency": ((n_bins, a, a), np.complex128), "magnitude": ((n_bins, a, a), np.float64),
              "multiple": ((n_bins, a), np.float64)}
    out = {name: mem.empty(*shapes[name]) for name in want}
    d_kept, d_given = mem.upload(np.ascontiguousarray(kept, dtype=np.int32)), mem.upload(np.ascontiguousarray(given, dtype=np.int32))
    fail = mem.zeros((2,), np.int32)
    _lib.check(_lib._handle().sc_partial_coherence_given_f64(mem.ptr(accum), n_bins, n_signals, _planes(mem, accum, planes), n_obs,
                                                             mem.ptr(d_kept), a, mem.ptr(d_given), len(given),
                                                             _ptr(mem, out.get("coherency")), _ptr(mem, out.get("magnitude")),
                                                             _ptr(mem, out.get("multiple")), mem.ptr(fail), mem.stream()),
               "sc_partial_coherence_given_f64")
    n_failed, n_explained = (int(n) for n in np.asarray(mem.download(fail)).ravel())
    return out, (n_failed, n_explained)


def _jackknife_workspace(mem, workspace_bytes, d, mask, over, n_units, unit_range):
    """(first unit, end unit, workspace or None, its bytes) of a jackknife call over ``unit_range`` (None: all ``n_units`` units of
    the spectra); ``workspace_bytes``: the entry-point family's sc_*_workspace_bytes, ``mask``: what it takes after the descriptor."""
    lo, hi = (0, n_units) if unit_range is None else unit_range
    ws_bytes = int(workspace_bytes(byref(d), mask, over, lo, hi))
    return lo, hi, (mem.empty((ws_bytes,), np.uint8) if ws_bytes else None), ws_bytes


def _jackknife(mem, prefix, spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq, unit_range):
    """jackknife / jackknife_phase: layout, unit range, workspace, output and the call of ``prefix`` + _f32 / _f64."""
    lib = _lib._handle()
    d = spectra.desc(expectation_type, n_freq)
    n_bins, n_units, unit_size, n_out = c_int64(), c_int64(), c_int64(), c_int64()
    _lib.check(getattr(lib, prefix + "_layout")(byref(d), measures, over, byref(n_bins), byref(n_units), byref(unit_size),
                                                byref(n_out)), prefix + "_layout")
    lo, hi, ws, ws_bytes = _jackknife_workspace(mem, getattr(lib, prefix + "_workspace_bytes"), d, measures, over, n_units.value,
                                                unit_range)
    out = mem.empty((n_out.value,), np.float64)
    fn = getattr(lib, prefix + ("_f64" if spectra.f64 else "_f32"))
    _lib.check(fn(mem.ptr(spectra.X), byref(d), mem.ptr(total), _planes(mem, total, planes), measures, over, lo, hi, n_units_total,
                  mem.ptr(out), _ptr(mem, ws), ws_bytes, mem.stream()), prefix)
    return out, n_bins.value


def jackknife(mem, spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq=None, unit_range=None):
    """Delete-one jackknife sums (sc_jackknife.hip): ONE pass over the complex64 / complex128 spectra (``spectra.X``, described by
    ``spectra.desc``) for every measure of the mask ``measures`` (_lib.JACKKNIFE_MEASURES) against the total CSM record ``total``
    (any rank's sum).  ``over``: _lib.JACKKNIFE_OVER; ``n_units_total``: delete units of the whole job; ``unit_range``: the units
    of these spectra to walk (default: all of them).  Returns (float64 device array laid out as _lib.jackknife_blocks says,
    n_bins)."""
    return _jackknife(mem, "sc_jackknife", spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq, unit_range)


def jackknife_phase(mem, spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq=None, unit_range=None):
    """Delete-one jackknife sums of the phase-lag family (jk_phase_kernel of sc_jackknife.hip): as ``jackknife``, with the mask
    ``measures`` of _lib.JACKKNIFE_PHASE_MEASURES and a total accumulator record ``total`` that holds the planes these measures
    read (_lib.JACKKNIFE_PHASE_PLANES) among its ``planes``.  Returns (float64 device array laid out as _lib.jackknife_blocks
    says, n_bins)."""
    return _jackknife(mem, "sc_jackknife_phase", spectra, expectation_type, total, planes, measures, over, n_units_total, n_freq,
                      unit_range)


def jackknife_phase_totals(mem, spectra, expectation_type, planes, over, n_freq=None, unit_range=None):
    """The total record of jackknife_phase from the spectra themselves (jk_phase_totals_kernel): float64 device array [n_bins,
    elements per bin] in the accumulator layout with the families ``planes``, the sums over the units ``unit_range`` of these
    spectra (default: all); the records of trial shards add.  Returns (record, n_observations of these spectra)."""
    from . import _stage_abc
    lib = _lib._handle()
    d = spectra.desc(expectation_type, n_freq)
    n_bins, per_bin, _, n_obs = _stage_abc.accum_layout(spectra, expectation_type, planes, n_freq)
    n_units = c_int64()
    _lib.check(lib.sc_jackknife_phase_layout(byref(d), 0x1, over, None, byref(n_units), None, None), "sc_jackknife_phase_layout")
    lo, hi, ws, ws_bytes = _jackknife_workspace(mem, lib.sc_jackknife_phase_totals_workspace_bytes, d, planes, over, n_units.value,
                                                unit_range)
    record = mem.empty((n_bins, per_bin), np.float64)
    fn = lib.sc_jackknife_phase_totals_f64 if spectra.f64 else lib.sc_jackknife_phase_totals_f32
    _lib.check(fn(mem.ptr(spectra.X), byref(d), planes, over, lo, hi, mem.ptr(record), _ptr(mem, ws), ws_bytes, mem.stream()),
               "sc_jackknife_phase_totals")
    return record, n_obs


def seed_connectivity(mem, spectra, expectation_type, seeds, targets, planes, measures, wide, n_freq=None, reduce=None,
                      n_observations=None):
    """Seed-based connectivity (sc_seed.hip): ONE pass over the complex64 / complex128 spectra (``spectra.X``, described by
    ``spectra.desc``) sums the seed record of ``planes`` (_lib.SEED_MEASURES) for the signals ``seeds`` against ``targets`` (int32
    arrays; None: every signal in order), then one small launch turns it into the ``measures`` (SC_M_* codes), each as doubles
    where its ``wide`` flag is set and floats otherwise.  The record is un-normalised, so trial shards add it: ``reduce`` (record
    -> record summed over the processes) and ``n_observations`` (local count -> the job's) are the caller's.  Returns the list of
    device arrays [n_bins, n_seeds, n_targets], in the order of ``measures``."""
    from . import _stage_abc
    lib = _lib._handle()
    d = spectra.desc(expectation_type, n_freq)
    n_seeds, n_targets = len(seeds), spectra.C if targets is None else len(targets)
    per_bin = c_int64()
    _lib.check(lib.sc_seed_record_layout(n_seeds, n_targets, planes, byref(per_bin)), "sc_seed_record_layout")
    n_bins, _, _, n_obs = _stage_abc.accum_layout(spectra, expectation_type, _lib.PLANE_CSM, n_freq)      # (the planes do not matter)
    d_seeds = mem.upload(np.ascontiguousarray(seeds, dtype=np.int32))
    d_targets = None if targets is None else mem.upload(np.ascontiguousarray(targets, dtype=np.int32))
    ws_bytes = int(lib.sc_seed_accumulate_workspace_bytes(byref(d), n_seeds, n_targets, planes))
    ws = mem.empty((ws_bytes,), np.uint8) if ws_bytes else None
    record = mem.empty((n_bins, per_bin.value), np.float64)
    fn = lib.sc_seed_accumulate_f64 if spectra.f64 else lib.sc_seed_accumulate_f32
    _lib.check(fn(mem.ptr(spectra.X), byref(d), mem.ptr(d_seeds), n_seeds, _ptr(mem, d_targets), n_targets, planes, mem.ptr(record),
                  _ptr(mem, ws), ws_bytes, mem.stream()), "sc_seed_accumulate")
    if reduce is not None:
        record = reduce(record)
    n_total = n_obs if n_observations is None else n_observations(n_obs)
    outs = [mem.empty((n_bins, n_seeds, n_targets), (np.complex128 if w else np.complex64) if m == _lib.M_COHERENCY else
                      (np.float64 if w else np.float32)) for m, w in zip(measures, wide)]
    n = len(measures)
    _lib.check(lib.sc_seed_measure_f64(mem.ptr(record), n_bins, mem.ptr(d_seeds), n_seeds, _ptr(mem, d_targets), n_targets, planes,
                                       n_total, n, (ctypes.c_int * n)(*measures), (ctypes.c_int * n)(*(int(bool(w)) for w in wide)),
                                       (ctypes.c_void_p * n)(*(mem.ptr(o).value for o in outs)), mem.stream()), "sc_seed_measure_f64")
    return outs



def _seed_jackknife_setup(mem, spectra, expectation_type, seeds, targets, n_freq):
    """(library, descriptor, n_seeds, n_targets, device seeds, device targets or None) of the two seed-jackknife drivers."""
    d = spectra.desc(expectation_type, n_freq)
    d_seeds = mem.upload(np.ascontiguousarray(seeds, dtype=np.int32))
    d_targets = None if targets is None else mem.upload(np.ascontiguousarray(targets, dtype=np.int32))
    return _lib._handle(), d, len(seeds), spectra.C if targets is None else len(targets), d_seeds, d_targets


def seed_jackknife_totals(mem, spectra, expectation_type, seeds, targets, planes, over, n_freq=None, unit_range=None):
    """The total record of seed_jackknife from the spectra themselves (sjk_kernel<TOTALS> of sc_seed_jackknife.hip): float64 device
    array [n_bins, sc_seed_record_layout doubles] with the families ``planes`` (_lib.SEED_JACKKNIFE_MEASURES), the sums over the
    units ``unit_range`` of these spectra (default: all) for ``seeds`` against ``targets`` (int32 arrays; None: every signal in
    order); the records of trial shards add."""
    lib, d, n_seeds, n_targets, d_seeds, d_targets = _seed_jackknife_setup(mem, spectra, expectation_type, seeds, targets, n_freq)
    per_bin, n_bins, n_units = c_int64(), c_int64(), c_int64()
    _lib.check(lib.sc_seed_record_layout(n_seeds, n_targets, planes, byref(per_bin)), "sc_seed_record_layout")
    _lib.check(lib.sc_seed_jackknife_layout(byref(d), n_seeds, n_targets, 0x1, over, byref(n_bins), byref(n_units), None, None),
               "sc_seed_jackknife_layout")
    lo, hi = (0, n_units.value) if unit_range is None else unit_range
    ws_bytes = int(lib.sc_seed_jackknife_totals_workspace_bytes(byref(d), n_seeds, n_targets, planes, over, lo, hi))
    ws = mem.empty((ws_bytes,), np.uint8) if ws_bytes else None
    record = mem.empty((n_bins.value, per_bin.value), np.float64)
    fn = lib.sc_seed_jackknife_totals_f64 if spectra.f64 else lib.sc_seed_jackknife_totals_f32
    _lib.check(fn(mem.ptr(spectra.X), byref(d), mem.ptr(d_seeds), n_seeds, _ptr(mem, d_targets), n_targets, planes, over, lo, hi,
                  mem.ptr(record), _ptr(mem, ws), ws_bytes, mem.stream()), "sc_seed_jackknife_totals")
    return record


def seed_jackknife(mem, spectra, expectation_type, seeds, targets, total, planes, measures, over, n_units_total, n_freq=None,
                   unit_range=None):
    """Delete-one jackknife sums of seed-based connectivity (sjk_kernel of sc_seed_jackknife.hip): ONE walk over the complex64 /
    complex128 spectra for every measure of the mask ``measures`` (_lib.SEED_JACKKNIFE_MEASURES) against the total record ``total``
    of seed_jackknife_totals (any rank's sum) with the families ``planes``.  ``over``, ``n_units_total``, ``unit_range``: as for
    ``jackknife``.  Returns (float64 device array: per measure of the mask, in table order, theta, sum d and sum d^2 as [n_bins,
    n_seeds, n_targets] each; n_bins)."""
    lib, d, n_seeds, n_targets, d_seeds, d_targets = _seed_jackknife_setup(mem, spectra, expectation_type, seeds, targets, n_freq)
    n_bins, n_units, n_out = c_int64(), c_int64(), c_int64()
    _lib.check(lib.sc_seed_jackknife_layout(byref(d), n_seeds, n_targets, measures, over, byref(n_bins), byref(n_units), None,
                                            byref(n_out)), "sc_seed_jackknife_layout")
    lo, hi = (0, n_units.value) if unit_range is None else unit_range
    ws_bytes = int(lib.sc_seed_jackknife_workspace_bytes(byref(d), n_seeds, n_targets, measures, over, lo, hi))
    ws = mem.empty((ws_bytes,), np.uint8) if ws_bytes else None
    out = mem.empty((n_out.value,), np.float64)
    fn = lib.sc_seed_jackknife_f64 if spectra.f64 else lib.sc_seed_jackknife_f32
    _lib.check(fn(mem.ptr(spectra.X), byref(d), mem.ptr(d_seeds), n_seeds, _ptr(mem, d_targets), n_targets, mem.ptr(total), planes,
                  measures, over, lo, hi, n_units_total, mem.ptr(out), _ptr(mem, ws), ws_bytes, mem.stream()), "sc_seed_jackknife")
    return out, n_bins.value
