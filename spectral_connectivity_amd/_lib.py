"""ctypes binding of the C ABI in include/sc_hip.h (libsc_hip.so).

The HIP library is the ONLY compute path of this package: if it cannot be loaded the import
of any compute entry point raises -- there is no NumPy/CPU fallback.

Two hosts sit on this binding.  The PyTorch host (engine.py: torch owns HBM buffers, streams and the RCCL collectives)
imports torch BEFORE the library on purpose: the PyTorch-ROCm wheel ships its own HIP runtime / rocFFT (same SONAMEs
as /opt/rocm); loading it first makes libsc_hip.so bind to that single runtime, so device pointers of torch tensors
are valid inside our kernels.  The NumPy host (numpy_host.py: memory, copies and streams through the library's own
sc_device_alloc / sc_memcpy_* / sc_stream_* calls) never imports torch; the library then binds to /opt/rocm's runtime.
One process uses one of the two: whichever loads the library first decides the runtime it is bound to.
"""
import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import sys

from . import _build

c_int64_p = POINTER(c_int64)

# ---- constants mirrored from include/sc_hip.h -------------------------------------------
SC_ABI_VERSION = 8
GRANGER_KEEP_OUTPUT = 1
CONDITIONAL_KEEP_OUTPUT = 1
BLOCKWISE_KEEP_OUTPUT = 1
DETREND = {None: 0, "constant": 1, "c": 1, "linear": 2, "l": 2}
MVAR_DTF, MVAR_DC, MVAR_PDC, MVAR_GPDC, MVAR_DDTF, MVAR_TRANSFER, MVAR_COEFFICIENTS, MVAR_NOISE_COVARIANCE = range(8)
PLANE_CSM, PLANE_ABS_IM, PLANE_IM_SQ, PLANE_SIGN_IM, PLANE_UNIT = 0x01, 0x02, 0x04, 0x08, 0x10
# axes of (window, trial, taper) an expectation type averages over (reference connectivity.py:67-75)
EXPECTATION_AXES = {
    "time": (0,),
    "trials": (1,),
    "tapers": (2,),
    "time_trials": (0, 1),
    "time_tapers": (0, 2),
    "trials_tapers": (1, 2),
    "time_trials_tapers": (0, 1, 2),
}
RECORD_F64 = 0x100          # OR-ed into `planes` when the records handed to a consumer hold doubles (float64 engine)
(M_POWER, M_CSM, M_COHERENCY, M_COHERENCE_MAGNITUDE, M_COHERENCE_PHASE, M_IMAGINARY_COHERENCE,
 M_PLV, M_PLI, M_WPLI, M_DEBIASED_PLI2, M_DEBIASED_WPLI2, M_PPC, M_PLV_COMPLEX) = range(13)
COMPLEX_MEASURES = {M_CSM, M_COHERENCY, M_PLV_COMPLEX}
MEASURE_PLANES = {
    M_POWER: PLANE_CSM, M_CSM: PLANE_CSM, M_COHERENCY: PLANE_CSM, M_COHERENCE_MAGNITUDE: PLANE_CSM,
    M_COHERENCE_PHASE: PLANE_CSM, M_IMAGINARY_COHERENCE: PLANE_CSM,
    M_PLV: PLANE_UNIT, M_PLV_COMPLEX: PLANE_UNIT, M_PPC: PLANE_UNIT,
    M_PLI: PLANE_SIGN_IM, M_DEBIASED_PLI2: PLANE_SIGN_IM,
    M_WPLI: PLANE_CSM | PLANE_ABS_IM, M_DEBIASED_WPLI2: PLANE_CSM | PLANE_ABS_IM | PLANE_IM_SQ,
}


class Timing(Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("ms", c_float)]


class SpectraDesc(Structure):
    _fields_ = [("n_freq", c_int64), ("n_windows", c_int64), ("n_trials", c_int64),
                ("n_tapers", c_int64), ("n_signals", c_int64), ("stride_freq", c_int64),
                ("stride_window", c_int64), ("stride_trial", c_int64), ("stride_taper", c_int64),
                ("reduce_window", c_int32), ("reduce_trial", c_int32), ("reduce_taper", c_int32),
                ("reserved", c_int32)]


# every symbol include/sc_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "sc_abi_version": (c_int, []),
    "sc_last_error": (c_char_p, []),
    "sc_device_count": (c_int, [POINTER(c_int)]),
    "sc_taper_windows_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                     c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sc_taper_windows_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                     c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sc_fft_plan_create_f64": (c_int, [POINTER(c_void_p), c_int64, c_int64]),
    "sc_fft_execute_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_accumulate_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_uint32, c_void_p, c_void_p]),
    "sc_measure_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_int, c_void_p, c_void_p]),
    "sc_measure_multi_f32": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_int, POINTER(c_int),
                                     POINTER(c_void_p), c_void_p]),
    "sc_measure_multi_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_int, POINTER(c_int),
                                     POINTER(c_void_p), c_void_p]),
    "sc_measure_multi_parts": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_uint32, c_int64, c_int,
                                       POINTER(c_int), POINTER(c_void_p), c_int, c_void_p]),
    "sc_measure_parts": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_uint32, c_int64, c_int, c_void_p, c_int, c_void_p]),
    "sc_timing_enable": (c_int, [c_int]),
    "sc_last_timing": (c_int, [POINTER(Timing), c_int, POINTER(c_int)]),
    "sc_multitaper_fft_supported": (c_int, [c_int64, c_int64]),
    "sc_fft_twiddles_f32": (c_int, [c_int64, c_void_p, c_void_p]),
    "sc_multitaper_fft_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                      c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "sc_timeseries_to_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "sc_multitaper_fft_f64_supported": (c_int, [c_int64, c_int64]),
    "sc_multitaper_fft_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                      c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "sc_fft_plan_create": (c_int, [POINTER(c_void_p), c_int64, c_int64]),
    "sc_fft_plan_work_bytes": (c_int, [c_void_p, POINTER(c_size_t)]),
    "sc_fft_execute": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_fft_plan_destroy": (c_int, [c_void_p]),
    "sc_accum_layout": (c_int, [POINTER(SpectraDesc), c_uint32, c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    "sc_csm_accumulate_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_void_p, c_void_p]),
    "sc_nonlinear_accumulate_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_uint32, c_void_p, c_void_p]),
    "sc_fused_supported": (c_int, [c_int64]),
    "sc_fused_csm_absim_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_void_p, c_void_p]),
    "sc_fused_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_uint32]),
    "sc_fused_csm_absim_ws_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_void_p, c_void_p, c_int64,
                                          c_void_p]),
    "sc_unit_scratch_bytes": (c_int64, [POINTER(SpectraDesc)]),
    "sc_unit_accumulate_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_fused_planes_covered": (c_uint32, [POINTER(SpectraDesc), c_uint32]),
    "sc_fused_sign_ws_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_fused_unit_scratch_bytes": (c_int64, [POINTER(SpectraDesc)]),
    "sc_fused_unit_ws_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_void_p, c_void_p, c_int64, c_void_p,
                                     c_int64, c_void_p]),
    "sc_planes_row_bytes": (c_int64, [c_int64]),
    "sc_multitaper_fft_planes_supported": (c_int, [c_int64, c_int64, c_int64]),
    "sc_multitaper_fft_planes_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                             c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_planes_scales_from_series_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_double, c_void_p, c_void_p, c_void_p]),
    "sc_planes_scales_work_bytes": (c_int64, [c_int64, c_int64]),
    "sc_planes_scales_quality_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_double, c_void_p, c_void_p, c_int64, c_void_p,
                                             c_void_p]),
    "sc_planes_scales_from_spectra_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "sc_planes_from_spectra_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_void_p, c_void_p]),
    "sc_spectra_from_planes_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_void_p, c_void_p]),
    "sc_fused2_supported": (c_int, [POINTER(SpectraDesc), c_uint32]),
    "sc_debug_fused2_clock": (c_int, [POINTER(c_double)]),
    "sc_debug_reload_env": (c_int, []),
    "sc_debug_fft_plans": (c_int, [POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "sc_fused2_csm_absim_parts_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_uint32, c_void_p, c_void_p, c_int64,
                                              POINTER(c_int), c_void_p]),
    "sc_fused2_csm_absim_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_uint32, c_void_p, c_void_p, c_int64,
                                        c_void_p]),
    "sc_comm_available": (c_int, []),
    "sc_comm_unique_id": (c_int, [c_void_p]),
    "sc_comm_create": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p)]),
    "sc_comm_destroy": (c_int, [c_void_p]),
    "sc_comm_size": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "sc_comm_allreduce_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_comm_exchange_blocks_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_comm_gather_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "sc_granger_workspace_bytes": (c_int, [c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "sc_granger_pairwise_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_uint32, c_int64,
                                        c_void_p, c_int64, c_double, c_int, c_void_p, c_size_t, c_int, c_void_p,
                                        c_void_p, c_void_p, POINTER(c_int32), c_void_p]),
    "sc_wilson_factor_f64": (c_int, [c_void_p, c_int64, c_int64, c_double, c_int, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p, POINTER(c_int32), c_void_p]),
    "sc_mvar_max_signals": (c_int, []),
    "sc_mvar_workspace_bytes": (c_int, [c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "sc_mvar_factor_f64": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_uint32, c_int64,
                                   c_double, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                   POINTER(c_int32), c_void_p]),
    "sc_mvar_measure_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_size_t,
                                    c_void_p]),
    "sc_conditional_granger_workspace_bytes": (c_int, [c_int64, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "sc_conditional_granger_f64": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_uint32, c_int64,
                                           c_void_p, c_void_p, c_int64, c_double, c_int, c_void_p, c_size_t, c_int,
                                           c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_void_p]),
    "sc_blockwise_granger_workspace_bytes": (c_int, [c_int64, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "sc_blockwise_granger_f64": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_uint32, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_double, c_int, c_void_p,
                                         c_size_t, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_int32), c_void_p]),
    "sc_global_coherence_max_signals": (c_int, []),
    "sc_global_coherence_f64": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_uint32, c_int64, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p]),
    "sc_canonical_max_group": (c_int, []),
    "sc_canonical_coherence_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_void_p,
                                           c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sc_imaginary_interaction_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_void_p,
                                             c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_interaction_vectors_lds_group": (c_int, [c_int]),
    "sc_imaginary_interaction_vectors_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_void_p,
                                                     c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_canonical_vectors_lds_group": (c_int, [c_int]),
    "sc_canonical_coherence_vectors_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_void_p,
                                                   c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_linear_dependence_max_joint": (c_int, []),
    "sc_linear_dependence_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_void_p,
                                         c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_partial_coherence_max_signals": (c_int, []),
    "sc_partial_coherence_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "sc_partial_given_max_given": (c_int, []),
    "sc_partial_given_max_kept": (c_int, []),
    "sc_partial_given_lds_bytes": (c_int64, [c_int64, c_int64]),
    "sc_partial_given_lds_limit": (c_int64, []),
    "sc_partial_coherence_given_f64": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_void_p, c_int, c_void_p, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sc_jackknife_layout": (c_int, [POINTER(SpectraDesc), c_uint32, c_int, c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    "sc_jackknife_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_uint32, c_int, c_int64, c_int64]),
    "sc_jackknife_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_uint32, c_uint32, c_int, c_int64, c_int64, c_int64,
                                 c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_jackknife_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_uint32, c_uint32, c_int, c_int64, c_int64, c_int64,
                                 c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_jackknife_phase_layout": (c_int, [POINTER(SpectraDesc), c_uint32, c_int, c_int64_p, c_int64_p, c_int64_p, c_int64_p]),
    "sc_jackknife_phase_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_uint32, c_int, c_int64, c_int64]),
    "sc_jackknife_phase_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_uint32, c_uint32, c_int, c_int64, c_int64, c_int64,
                                       c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_jackknife_phase_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_uint32, c_uint32, c_int, c_int64, c_int64, c_int64,
                                       c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_jackknife_phase_totals_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_uint32, c_int, c_int64, c_int64]),
    "sc_jackknife_phase_totals_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_int, c_int64, c_int64, c_void_p, c_void_p,
                                              c_int64, c_void_p]),
    "sc_jackknife_phase_totals_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_uint32, c_int, c_int64, c_int64, c_void_p, c_void_p,
                                              c_int64, c_void_p]),
    "sc_seed_connectivity_max_seeds": (c_int, []),
    "sc_seed_record_layout": (c_int, [c_int64, c_int64, c_uint32, c_int64_p]),
    "sc_seed_accumulate_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_int64, c_int64, c_uint32]),
    "sc_seed_accumulate_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_int64, c_void_p, c_int64, c_uint32, c_void_p,
                                       c_void_p, c_int64, c_void_p]),
    "sc_seed_accumulate_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_int64, c_void_p, c_int64, c_uint32, c_void_p,
                                       c_void_p, c_int64, c_void_p]),
    "sc_seed_measure_f64": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_uint32, c_int64, c_int,
                                    POINTER(c_int), POINTER(c_int), POINTER(c_void_p), c_void_p]),
    "sc_seed_jackknife_layout": (c_int, [POINTER(SpectraDesc), c_int64, c_int64, c_uint32, c_int, c_int64_p, c_int64_p, c_int64_p,
                                         c_int64_p]),
    "sc_seed_jackknife_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_int64, c_int64, c_uint32, c_int, c_int64, c_int64]),
    "sc_seed_jackknife_totals_workspace_bytes": (c_int64, [POINTER(SpectraDesc), c_int64, c_int64, c_uint32, c_int, c_int64, c_int64]),
    "sc_seed_jackknife_totals_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_int64, c_void_p, c_int64, c_uint32, c_int,
                                             c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_seed_jackknife_totals_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_int64, c_void_p, c_int64, c_uint32, c_int,
                                             c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_seed_jackknife_f32": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_uint32,
                                      c_uint32, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_seed_jackknife_f64": (c_int, [c_void_p, POINTER(SpectraDesc), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_uint32,
                                      c_uint32, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_measure_f32": (c_int, [c_void_p, c_int64, c_int64, c_uint32, c_int64, c_int, c_void_p, c_void_p]),
    # host-pointer side (sc_memory.hip)
    "sc_device_alloc": (c_int, [POINTER(c_void_p), c_size_t, c_void_p]),
    "sc_device_free": (c_int, [c_void_p, c_void_p]),
    "sc_host_alloc": (c_int, [POINTER(c_void_p), c_size_t]),
    "sc_host_free": (c_int, [c_void_p]),
    "sc_host_register": (c_int, [c_void_p, c_size_t]),
    "sc_host_unregister": (c_int, [c_void_p]),
    "sc_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "sc_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "sc_memset_zero": (c_int, [c_void_p, c_size_t, c_void_p]),
    "sc_stream_create": (c_int, [POINTER(c_void_p)]),
    "sc_stream_destroy": (c_int, [c_void_p]),
    "sc_stream_synchronize": (c_int, [c_void_p]),
    "sc_nonfinite_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "sc_nonfinite_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "sc_amplitude_range_work_bytes": (c_int64, [c_int64, c_int64]),
    "sc_amplitude_range_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sc_spectra_widen_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
}

_lib = None
_bound_with_torch = None        # True / False once the library is loaded: which HIP runtime it is bound to


class HipEngineError(RuntimeError):
    """A libsc_hip.so entry point returned a negative status."""


def record_planes(planes, f64):
    """`planes` as the consumers of accumulator records want it: with RECORD_F64 when the records hold doubles."""
    return (planes | RECORD_F64) if f64 else (planes & ~RECORD_F64)


# workspace bounds of the chunked stage-D drivers (_stage_d.py), read at call time
GRANGER_WORK_BYTES = 8 << 30        # one sc_granger_pairwise_f64 call (160 bytes per problem and bin; the pairs go in chunks)
CONDITIONAL_WORK_BYTES = 4 << 30    # one sc_conditional_granger_f64 / sc_blockwise_granger_f64 call (dropped signals / block pairs in chunks)


def conditional_chunk(n_groups, n_signals, workspace_bytes, cap=None):
    """Dropped signals per sc_conditional_granger_f64 call (both hosts): as many as keep the workspace under ``cap`` -- at least
    one, at most n_signals and at most 65535 reduced problems.  ``workspace_bytes(n_dropped)``: the library's query."""
    cap = CONDITIONAL_WORK_BYTES if cap is None else cap
    one = workspace_bytes(1)
    per = max(1, workspace_bytes(2) - one)
    return int(max(1, min(n_signals, 65535 // n_groups, (cap - (one - per)) // per)))


def blockwise_chunk(n_groups, n_pairs, workspace_bytes, cap=None):
    """Block pairs per sc_blockwise_granger_f64 call (both hosts), among ``n_pairs`` pairs of one size m: as many as keep the
    workspace under ``cap`` (CONDITIONAL_WORK_BYTES) -- at least one, at most 65535 problems.  ``workspace_bytes(n)``: the
    library's query for n pairs."""
    return conditional_chunk(n_groups, n_pairs, workspace_bytes, cap)


def blockwise_pairs(group_labels, n_signals, max_signals):
    """Labels of blockwise_spectral_granger_prediction, checked before any device work (both hosts): (labels, pairs).
    ``labels`` = np.unique of ``group_labels``; ``pairs`` the unordered block pairs a < b as (members [m] int32: the signals of
    a, then of b; n_a; (a, b)).  ValueError for a label list of the wrong length, fewer than two blocks and a pair of more than
    ``max_signals`` signals."""
    import numpy as np
    group_labels = np.asarray(group_labels)
    if group_labels.ndim != 1 or len(group_labels) != n_signals:
        raise ValueError(f"group_labels must have one label per signal ({n_signals}), got {group_labels.shape}")
    labels = np.unique(group_labels)
    if len(labels) < 2:
        raise ValueError(f"blockwise Granger needs at least two groups of signals (got {len(labels)})")
    blocks = [np.flatnonzero(group_labels == lab) for lab in labels]
    pairs = []
    for a in range(len(blocks)):
        for b in range(a + 1, len(blocks)):
            m = len(blocks[a]) + len(blocks[b])
            if m > max_signals:
                raise ValueError(f"blockwise Granger: groups {labels[a].item()!r} and {labels[b].item()!r} have {m} signals together; "
                                 f"a group pair supports at most {max_signals}")
            pairs.append((np.concatenate([blocks[a], blocks[b]]).astype(np.int32), len(blocks[a]), (a, b)))
    return labels, pairs


def blockwise_batches(pairs, n_obs):
    """The pairs of blockwise_pairs grouped by m = n_a + n_b: (batches, n_skipped), ``batches`` maps m (ascending) to
    (members [n][m], split [n], cell [n][2]) int32 arrays.  A pair of more signals than the ``n_obs`` observations has a
    rank-deficient spectrum: it is left out (NaN) and counted in ``n_skipped``."""
    import numpy as np
    by_m, n_skipped = {}, 0
    for members, na, cell in pairs:
        if len(members) > n_obs:
            n_skipped += 1
            continue
        by_m.setdefault(len(members), []).append((members, na, cell))
    batches = {}
    for m, items in sorted(by_m.items()):
        batches[m] = (np.stack([it[0] for it in items]).astype(np.int32), np.array([it[1] for it in items], dtype=np.int32),
                      np.array([it[2] for it in items], dtype=np.int32))
    return batches, n_skipped


BLOCK_SIGNALS = 128        # channel block of the tiling of more than 256 signals (a multiple of the 16-channel record tile)


def tile_plan(n_signals, block=BLOCK_SIGNALS):
    """Stage B for MORE signals than one launch of the kernels stages (256), both hosts: the channels are cut into blocks of
    ``block``, every pair of blocks (a < b) is accumulated as a request of its own (<= 256 signals) and its 16 x 16 record tiles
    are copied to their places in the full record.  Yields (a, b, cols, src, dst) per block pair: ``cols`` the channels of the
    request (block a, then block b), ``src`` the tiles of its record to keep and ``dst`` their indices in the full record (tile
    (bi, bj), bi <= bj, of a record of nb tile rows has index bi nb - bi (bi - 1) / 2 + (bj - bi): include/sc_hip.h).  The cross
    tiles of (a, b) come from that pair, the tiles inside block a from the pair (a, a + 1), those inside the last block from the
    last pair -- every tile of the full record exactly once."""
    import numpy as np

    def tile(bi, bj, nb):
        return bi * nb - bi * (bi - 1) // 2 + (bj - bi)

    n_blk, NB, per = -(-n_signals // block), -(-n_signals // 16), block // 16
    for a in range(n_blk - 1):
        for b in range(a + 1, n_blk):
            cols = np.concatenate([np.arange(a * block, (a + 1) * block), np.arange(b * block, min((b + 1) * block, n_signals))])
            nb_s = -(-len(cols) // 16)
            src, dst = [], []
            for ti in range(nb_s):
                for tj in range(ti, nb_s):
                    in_a_i, in_a_j = ti < per, tj < per
                    if in_a_i and in_a_j:
                        keep = b == a + 1                                   # inside block a: from its first partner
                    elif not in_a_i and not in_a_j:
                        keep = a == n_blk - 2 and b == n_blk - 1            # inside the last block: from the last pair
                    else:
                        keep = True                                         # cross tiles of (a, b)
                    if keep:
                        gi = a * per + ti if in_a_i else b * per + (ti - per)
                        gj = a * per + tj if in_a_j else b * per + (tj - per)
                        src.append(tile(ti, tj, nb_s))
                        dst.append(tile(gi, gj, NB))
            yield a, b, cols, src, dst


def member_stride(max_group_size):
    """Row length of the member table of sc_canonical_coherence_f64 / sc_imaginary_interaction_f64 for groups of at most
    ``max_group_size`` channels (include/sc_hip.h): 16, 32 or 128."""
    return 16 if max_group_size <= 16 else (32 if max_group_size <= 32 else 128)


def member_table(groups):
    """(members int32 [G][stride] channel indices, -1 padded; sizes int32 [G]; stride) of the int arrays ``groups``."""
    import numpy as np
    sizes = np.array([len(g) for g in groups], dtype=np.int32)
    stride = member_stride(int(sizes.max()))
    members = np.full((len(groups), stride), -1, dtype=np.int32)
    for i, g in enumerate(groups):
        members[i, :len(g)] = g
    return members, sizes, stride


def interaction_groups(group_labels, n_signals, max_group):
    """Labels of maximized_imaginary_coherence / multivariate_interaction_measure, checked before any device work (both hosts):
    (labels, members, sizes, stride) -- ``labels`` = np.unique of ``group_labels``, then member_table of the groups in that
    order.  ValueError for a label list of the wrong length, fewer than two groups and a group of more than ``max_group``
    channels (sc_canonical_max_group())."""
    labels, groups = _labelled_groups(group_labels, n_signals)
    for lab, g in zip(labels, groups):
        if len(g) > max_group:
            raise ValueError(f"imaginary interaction: group {lab.item()!r} has {len(g)} channels; a group may have at most "
                             f"{max_group}")
    return (labels,) + member_table(groups)


def _labelled_groups(group_labels, n_signals):
    """(np.unique of the labels, the channel indices of every group) after the label checks of interaction_groups."""
    import numpy as np
    group_labels = np.asarray(group_labels)
    if group_labels.ndim != 1 or len(group_labels) != n_signals:
        raise ValueError(f"group_labels must have one label per signal ({n_signals}), got {group_labels.shape}")
    labels = np.unique(group_labels)
    if len(labels) < 2:
        raise ValueError(f"imaginary interaction needs at least two groups of signals (got {len(labels)})")
    return labels, [np.flatnonzero(group_labels == lab) for lab in labels]


def dependence_groups(group_labels, n_signals, max_joint):
    """Labels of linear_dependence, checked before any device work (both hosts): (labels, members, sizes, stride) as
    interaction_groups, with its label checks and messages.  ``group_labels`` None: every signal is its own group, labels =
    np.arange(n_signals).  ValueError for a pair of groups with more than ``max_joint`` signals together
    (sc_linear_dependence_max_joint()): the two largest groups decide."""
    import numpy as np
    if group_labels is None:
        if n_signals < 2:
            raise ValueError(f"linear dependence needs at least two signals (got {n_signals})")
        labels, groups = np.arange(n_signals), [np.array([c]) for c in range(n_signals)]
    else:
        labels, groups = _labelled_groups(group_labels, n_signals)
    if len(groups) >= 2:
        a, b = sorted(np.argsort([len(g) for g in groups], kind="stable")[-2:].tolist())
        m = len(groups[a]) + len(groups[b])
        if m > max_joint:
            raise ValueError(f"linear dependence: groups {labels[a].item()!r} and {labels[b].item()!r} have {m} signals together; "
                             f"a pair of groups may have at most {max_joint}")
    return (labels,) + member_table(groups)


def dependence_rank_skipped(sizes, n_obs):
    """Number of group pairs with more signals together than the ``n_obs`` observations: their joint cross-spectral matrix is
    singular and the device leaves them NaN."""
    import numpy as np
    s = np.asarray(sizes, dtype=np.int64)
    over = (s[:, None] + s[None, :]) > n_obs
    return int(np.triu(over, 1).sum())


def interaction_kept(sizes, n_obs):
    """Groups whose real cross-spectral block can be positive definite: Re S_gg has rank at most 2 n_obs, so the groups of more
    channels are left out (NaN) before any device work -- the kernels' Cholesky may round such a block to a tiny positive pivot.
    Returns (indices of the kept groups, number left out)."""
    import numpy as np
    keep = np.flatnonzero(np.asarray(sizes) <= 2 * n_obs)
    return keep, len(sizes) - len(keep)


def _index_list(values, what, n_signals):
    """1-D int64 array of distinct signal indices in [0, n_signals) out of ``values``; ValueError otherwise."""
    import numpy as np
    raw = np.asarray(values)
    if raw.ndim != 1:
        raise ValueError(f"partial coherence: `{what}` must be a list of signal indices (got shape {raw.shape})")
    if raw.size and (raw.dtype == bool or not np.issubdtype(raw.dtype, np.integer)):
        raise ValueError(f"partial coherence: `{what}` must hold integer signal indices (got {raw.dtype})")
    idx = raw.astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n_signals):
        raise ValueError(f"partial coherence: `{what}` has an index outside [0, {n_signals})")
    if len(np.unique(idx)) != len(idx):
        raise ValueError(f"partial coherence: `{what}` names a signal twice")
    return idx


def partial_given_indices(given, signals, n_signals):
    """The two index lists of partial and multiple coherence given a chosen set, checked before any device work (both hosts):
    (kept int32 [a] in the order of ``signals``, given int32 [m] in the caller's order).  ``signals`` None: every signal that is
    not given, ascending.  ValueError for an empty ``given`` (or ``signals`` without ``given``), an empty kept set, duplicates,
    overlap between the two lists, an index outside [0, n_signals) and anything but integers."""
    import numpy as np
    if given is None:
        raise ValueError("partial coherence: `signals` needs `given`, the signals to condition on")
    z = _index_list(given, "given", n_signals)
    if len(z) == 0:
        raise ValueError("partial coherence: `given` is empty (without the keyword, every other signal is conditioned on)")
    if signals is None:
        kept = np.setdiff1d(np.arange(n_signals), z)
    else:
        kept = _index_list(signals, "signals", n_signals)
        both = np.intersect1d(kept, z)
        if len(both):
            raise ValueError(f"partial coherence: signals {both.tolist()} are both kept and given")
    if len(kept) == 0:
        raise ValueError("partial coherence: no signal is kept")
    return kept.astype(np.int32), z.astype(np.int32)


# ---- delete-one jackknife (sc_jackknife.hip): the request, checked before any device work (both hosts) ----------------------------
# measure name -> (bit of the `measures` mask of sc_jackknife_*, variance-stabilising transform, entries per bin: 1 = C, 2 = C x C);
# dict order = order of the blocks in the library's output
JACKKNIFE_MEASURES = {
    "power": (0x1, "log", 1),
    "coherence_magnitude": (0x2, "fisher_z", 2),
    "imaginary_coherence": (0x4, "identity", 2),
}
JACKKNIFE_OVER = {"trials": 0, "observations": 1}


def _jackknife_names(measures, *tables):
    """The measure list ``measures`` (a name or an iterable of names) as a tuple; ValueError -- with the names of ``tables``
    spelled out -- for an empty list and a name none of the tables has."""
    measures = (measures,) if isinstance(measures, str) else tuple(measures)
    valid = ", ".join(repr(k) for table in tables for k in table)
    if not measures:
        raise ValueError(f"jackknife: measures is empty; choose from {valid}")
    unknown = [m for m in measures if not any(m in table for table in tables)]
    if unknown:
        raise ValueError(f"jackknife: unknown measure {unknown[0]!r}; choose from {valid}")
    return measures


def jackknife_request(measures, over, expectation_type, n_trials, n_observations):
    """(names in output order, measures mask, `over` code, n_units) of Connectivity.jackknife; ValueError -- with the valid choices
    spelled out -- for an empty or unknown measure list, a bad ``over``, an expectation that keeps the trial axis with
    over="trials", and fewer than two delete units.  ``n_trials`` / ``n_observations``: of the whole job."""
    measures = _jackknife_names(measures, JACKKNIFE_MEASURES)
    if over not in JACKKNIFE_OVER:
        raise ValueError(f"jackknife: over must be 'trials' or 'observations' (got {over!r})")
    if over == "trials":
        if 1 not in EXPECTATION_AXES[expectation_type]:
            ok = ", ".join(repr(k) for k, axes in EXPECTATION_AXES.items() if 1 in axes)
            raise ValueError(f"jackknife over trials needs an expectation_type that averages over trials ({ok}), got "
                             f"{expectation_type!r}; use over='observations'")
        n_units = int(n_trials)
        if n_units < 2:
            raise ValueError(f"jackknife over trials needs n_trials >= 2 (got {n_units}); use over='observations'")
    else:
        n_units = int(n_observations)
        if n_units < 2:
            raise ValueError(f"jackknife over observations needs n_observations >= 2 (got {n_units} with expectation_type "
                             f"{expectation_type!r})")
    names = [k for k in JACKKNIFE_MEASURES if k in measures]
    mask = 0
    for k in names:
        mask |= JACKKNIFE_MEASURES[k][0]
    return names, mask, JACKKNIFE_OVER[over], n_units


# the phase-lag family (jk_phase_kernel, sc_jackknife_phase_*): a mask of its own, same tuple; all on the identity scale
JACKKNIFE_PHASE_MEASURES = {
    "phase_lag_index": (0x1, "identity", 2),
    "weighted_phase_lag_index": (0x2, "identity", 2),
    "debiased_squared_phase_lag_index": (0x4, "identity", 2),
    "debiased_squared_weighted_phase_lag_index": (0x8, "identity", 2),
}
# planes of the total record each of them reads (= MEASURE_PLANES of the measure's own method)
JACKKNIFE_PHASE_PLANES = {
    "phase_lag_index": PLANE_SIGN_IM, "debiased_squared_phase_lag_index": PLANE_SIGN_IM,
    "weighted_phase_lag_index": PLANE_CSM | PLANE_ABS_IM,
    "debiased_squared_weighted_phase_lag_index": PLANE_CSM | PLANE_ABS_IM | PLANE_IM_SQ,
}


def jackknife_split(measures):
    """(old names, phase-lag names) of a measure list of Connectivity.jackknife, as given; ValueError -- all seven names spelled
    out -- for an empty list and an unknown name."""
    measures = _jackknife_names(measures, JACKKNIFE_MEASURES, JACKKNIFE_PHASE_MEASURES)
    return (tuple(m for m in measures if m in JACKKNIFE_MEASURES), tuple(m for m in measures if m in JACKKNIFE_PHASE_MEASURES))


def jackknife_phase_request(measures, over, expectation_type, n_trials, n_observations):
    """jackknife_request for the phase-lag family: (names in output order, sc_jackknife_phase_* mask, `over` code, n_units, planes
    the total record must hold).  The same ValueErrors, and one more: the two debiased measures need at least two observations in
    a delete-one set, n' = (n_units - 1) g >= 2 -- violated only by two units of one observation each."""
    measures = _jackknife_names(measures, JACKKNIFE_PHASE_MEASURES)
    _, _, over_id, n_units = jackknife_request(("imaginary_coherence",), over, expectation_type, n_trials, n_observations)
    names = [k for k in JACKKNIFE_PHASE_MEASURES if k in measures]
    unit_size = int(n_observations) // n_units if over == "trials" else 1
    if (n_units - 1) * unit_size < 2 and any(k.startswith("debiased") for k in names):
        raise ValueError("jackknife: the debiased phase-lag measures need at least two observations in a delete-one set, "
                         f"(n_units - 1) x observations per unit >= 2 (got {n_units} units of {unit_size})")
    mask = planes = 0
    for k in names:
        mask |= JACKKNIFE_PHASE_MEASURES[k][0]
        planes |= JACKKNIFE_PHASE_PLANES[k]
    return names, mask, over_id, n_units, planes


def jackknife_blocks(names, n_bins, n_signals):
    """[(name, first double, doubles per array, array shape)] of the library's output for the measures ``names`` (output order;
    all of JACKKNIFE_MEASURES or all of JACKKNIFE_PHASE_MEASURES: one call's): every block is three arrays -- theta(S), sum d,
    sum d^2."""
    out, at = [], 0
    for k in names:
        rank = (JACKKNIFE_MEASURES.get(k) or JACKKNIFE_PHASE_MEASURES[k])[2]
        shape = (n_bins, n_signals) if rank == 1 else (n_bins, n_signals, n_signals)
        size = n_bins * n_signals ** rank
        out.append((k, at, size, shape))
        at += 3 * size
    return out, at


# ---- seed-based connectivity (sc_seed.hip): the request, checked before any device work (both hosts) -------------------------------
SEED_PLANE_POWER = 0x20          # SC_SEED_PLANE_POWER: sum |x_seed|^2, sum |x_target|^2 of a seed record
# measure name -> (SC_M_* code of sc_seed_measure_f64, planes of the seed record it reads)
SEED_MEASURES = {
    "coherency": (M_COHERENCY, PLANE_CSM | SEED_PLANE_POWER),
    "coherence_magnitude": (M_COHERENCE_MAGNITUDE, PLANE_CSM | SEED_PLANE_POWER),
    "coherence_phase": (M_COHERENCE_PHASE, PLANE_CSM | SEED_PLANE_POWER),
    "imaginary_coherence": (M_IMAGINARY_COHERENCE, PLANE_CSM | SEED_PLANE_POWER),
    "phase_locking_value": (M_PLV, PLANE_UNIT),
    "pairwise_phase_consistency": (M_PPC, PLANE_UNIT),
    "phase_lag_index": (M_PLI, PLANE_SIGN_IM),
    "weighted_phase_lag_index": (M_WPLI, PLANE_CSM | PLANE_ABS_IM),
    "debiased_squared_phase_lag_index": (M_DEBIASED_PLI2, PLANE_SIGN_IM),
    "debiased_squared_weighted_phase_lag_index": (M_DEBIASED_WPLI2, PLANE_CSM | PLANE_ABS_IM | PLANE_IM_SQ),
}


def seed_record_doubles(n_seeds, n_targets, planes):
    """Doubles per bin of a seed record (sc_seed_record_layout restated): two planes for the cross-spectrum and for the unit
    phasors, one for each other family, [n_seeds][n_targets] each, then the two power vectors."""
    n_planes = sum(width for bit, width in ((PLANE_CSM, 2), (PLANE_ABS_IM, 1), (PLANE_IM_SQ, 1), (PLANE_SIGN_IM, 1), (PLANE_UNIT, 2))
                   if planes & bit)
    return n_planes * n_seeds * n_targets + ((n_seeds + n_targets) if planes & SEED_PLANE_POWER else 0)


def _seed_indices(values, what, n_signals):
    import numpy as np
    arr = np.asarray(values)
    if arr.ndim != 1 or arr.size == 0:
        raise ValueError(f"seed_connectivity: {what} must be a non-empty list of signal indices")
    if arr.dtype == bool or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"seed_connectivity: {what} must be integers (got {arr.dtype})")
    bad = (arr < 0) | (arr >= n_signals)
    if bad.any():
        raise ValueError(f"seed_connectivity: {what} index {int(arr[bad][0])} is outside [0, {n_signals})")
    if len(np.unique(arr)) != arr.size:
        raise ValueError(f"seed_connectivity: {what} holds an index twice")
    return arr.astype(np.int32)


def seed_request(seeds, targets, measures, n_signals, max_seeds):
    """(seeds int32, targets int32 or None for all signals in order, names in the order asked, SC_M_* codes, planes of the record)
    of Connectivity.seed_connectivity; ValueError -- with the valid choices spelled out -- for an unknown, empty or repeated
    measure, an empty list, an index that is out of range, not an integer or repeated, and more than ``max_seeds`` seeds."""
    measures = [measures] if isinstance(measures, str) else list(measures)
    valid = ", ".join(SEED_MEASURES)
    if not measures:
        raise ValueError(f"seed_connectivity: measures is empty; choose from {valid}")
    unknown = [m for m in measures if m not in SEED_MEASURES]
    if unknown:
        raise ValueError(f"seed_connectivity: unknown measure {unknown[0]!r}; choose from {valid}")
    if len(set(measures)) != len(measures):
        raise ValueError(f"seed_connectivity: a measure is asked for twice ({measures})")
    seeds = _seed_indices(seeds, "seeds", n_signals)
    if len(seeds) > max_seeds:
        raise ValueError(f"seed_connectivity: at most {max_seeds} seeds per call (got {len(seeds)})")
    if targets is not None:
        targets = _seed_indices(targets, "targets", n_signals)
    planes = 0
    for m in measures:
        planes |= SEED_MEASURES[m][1]
    return seeds, targets, measures, [SEED_MEASURES[m][0] for m in measures], planes


# ---- delete-one jackknife of seed-based connectivity (sc_seed_jackknife.hip): the request, checked before any device work -----------
# measure name -> (bit of the `measures` mask of sc_seed_jackknife_*, transform, planes of the total record it reads); dict order =
# order of the blocks in the library's output: the pair measures of JACKKNIFE_MEASURES, then JACKKNIFE_PHASE_MEASURES
SEED_JACKKNIFE_MEASURES = {
    "coherence_magnitude": (0x1, "fisher_z", PLANE_CSM | SEED_PLANE_POWER),
    "imaginary_coherence": (0x2, "identity", PLANE_CSM | SEED_PLANE_POWER),
    "phase_lag_index": (0x4, "identity", PLANE_SIGN_IM),
    "weighted_phase_lag_index": (0x8, "identity", PLANE_CSM | PLANE_ABS_IM),
    "debiased_squared_phase_lag_index": (0x10, "identity", PLANE_SIGN_IM),
    "debiased_squared_weighted_phase_lag_index": (0x20, "identity", PLANE_CSM | PLANE_ABS_IM | PLANE_IM_SQ),
}


def seed_jackknife_request(seeds, targets, measures, over, expectation_type, n_trials, n_observations, n_signals, max_seeds):
    """(seeds int32, targets int32 or None for all signals in order, names in output order, sc_seed_jackknife_* mask, planes of the
    total record, `over` code, n_units) of Connectivity.seed_jackknife: the index rules of seed_request and the rules of
    jackknife_request / jackknife_phase_request, each checked by its own function.  ValueError for what they refuse, for "power"
    (not a pair measure) and for a measure asked for twice."""
    old, new = jackknife_split(measures)
    if "power" in old:
        raise ValueError("seed_jackknife: 'power' is not a measure of a (seed, target) pair; choose from "
                         + ", ".join(repr(k) for k in SEED_JACKKNIFE_MEASURES) + " (Connectivity.jackknife has the power)")
    if len(set(old + new)) != len(old + new):
        raise ValueError(f"seed_jackknife: a measure is asked for twice ({list(old + new)})")
    plans = [jackknife_request(old, over, expectation_type, n_trials, n_observations)] if old else []
    if new:
        plans.append(jackknife_phase_request(new, over, expectation_type, n_trials, n_observations))
    seeds, targets = seed_request(seeds, targets, ("coherency",), n_signals, max_seeds)[:2]
    asked = {k for plan in plans for k in plan[0]}
    names = [k for k in SEED_JACKKNIFE_MEASURES if k in asked]
    mask = planes = 0
    for k in names:
        mask |= SEED_JACKKNIFE_MEASURES[k][0]
        planes |= SEED_JACKKNIFE_MEASURES[k][2]
    return seeds, targets, names, mask, planes, plans[0][2], plans[0][3]


def library_path():
    return os.environ.get("SC_HIP_LIB", _build.LIB)


def load(torch_host=None):
    """Load (building in-tree if the sources are newer) and type libsc_hip.so.  Raises if impossible.
    ``torch_host``: the caller hands torch tensors' device pointers to the library, so torch's HIP runtime must be the
    one the library binds to (torch imported first); numpy_host passes False and never imports torch.  None: whatever the host of
    this process is (SC_HIP_HOST, _hosts.py)."""
    global _lib, _bound_with_torch
    if torch_host is None:
        from . import _hosts
        torch_host = _hosts.kind() != "numpy"
    if _lib is not None:
        if torch_host and not _bound_with_torch:
            raise RuntimeError(
                "libsc_hip.so was loaded by the NumPy host (spectral_connectivity_amd.numpy_host) and is bound to "
                "/opt/rocm's HIP runtime; the PyTorch host cannot share it in the same process (torch ships its own "
                "runtime). Import spectral_connectivity_amd (or torch) before numpy_host, or use separate processes.")
        return _lib
    if torch_host or "torch" in sys.modules:
        import torch  # noqa: F401  (must precede CDLL, see module docstring)
    path = library_path()
    if path == _build.LIB and _build.is_stale():
        try:
            _build.build(verbose=False)
        except Exception as exc:  # no hipcc, compile error: fail loudly, no CPU fallback
            if not os.path.exists(path):
                raise RuntimeError(
                    "spectral_connectivity_amd needs its HIP extension libsc_hip.so and could not "
                    f"build it ({exc}). Run `python -m spectral_connectivity_amd._build` on a machine "
                    "with ROCm's hipcc; there is no CPU fallback.") from exc
    try:
        lib = ctypes.CDLL(path)
    except OSError as exc:
        raise RuntimeError(f"cannot load HIP extension {path}: {exc}. There is no CPU fallback.") from exc
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.sc_abi_version() != SC_ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.sc_abi_version()} != {SC_ABI_VERSION}")
    _lib = lib
    _bound_with_torch = "torch" in sys.modules
    return lib


def _handle():
    """The loaded library, whichever host loaded it (the PyTorch host's load() on first use otherwise)."""
    return _lib if _lib is not None else load()


def check(status, what=""):
    if status != 0:
        msg = _handle().sc_last_error()
        raise HipEngineError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")


def reload_debug_env():
    """The library reads its diagnostic switches (SC_FUSED_DEBUG, SC_FUSED_SPLIT, SC_WILSON_FFT, ...) from the environment once,
    when it is loaded; tools and tests that change one afterwards call this (no-op while the library is not loaded)."""
    if _lib is not None:
        _lib.sc_debug_reload_env()


def fft_plan_counts():
    """(rocfft_plan_create calls of the process, plans the library's pools hold, idle real-to-complex row plans among them): rocFFT
    plans are pooled by geometry and never destroyed (sc_fft_plan_destroy), so the first two are always equal and grow with the
    DISTINCT geometries only."""
    a, b, c = c_int64(0), c_int64(0), c_int64(0)
    check(_handle().sc_debug_fft_plans(byref(a), byref(b), byref(c)), "sc_debug_fft_plans")
    return a.value, b.value, c.value


def set_debug_env(name, value):
    """os.environ[name] = value (None: unset) and have the library see it."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    reload_debug_env()


def device_count():
    n = c_int(0)
    check(_handle().sc_device_count(byref(n)), "sc_device_count")
    return n.value


ENABLE_GPU_ENV = "SPECTRAL_CONNECTIVITY_ENABLE_GPU"


def gpu_switch():
    """The reference's import-time backend switch (transforms.py:405-439, connectivity.py:31-65,
    minimum_phase_decomposition.py:14-26), read the way the reference reads it: the string "true" asks for the GPU
    backend, anything else for NumPy.  Returns True ("true": the HIP engine was asked for by name), None (unset: this
    package only has the HIP engine, nothing to choose) or False (set to something else: the caller asked for the
    CPU path, which this package does not have)."""
    v = os.environ.get(ENABLE_GPU_ENV)
    return None if v is None else v == "true"


def honour_gpu_switch():
    """Import-time half of the switch (called from transforms.py like the reference's module-level block): with
    SPECTRAL_CONNECTIVITY_ENABLE_GPU=true the engine must be there NOW -- a missing / unbuildable libsc_hip.so raises
    RuntimeError at import, like the reference's missing CuPy does (transforms.py:429-434)."""
    if gpu_switch():
        try:
            load()
        except Exception as exc:
            raise RuntimeError(
                f"GPU support was explicitly requested via {ENABLE_GPU_ENV}='true', but the HIP engine "
                f"libsc_hip.so could not be loaded ({exc}). Build it with "
                "'python -m spectral_connectivity_amd._build' on a machine with ROCm's hipcc.") from exc


def require_gpu():
    """The product path runs on an MI355X only: fail loudly when none is visible."""
    if gpu_switch() is False:
        raise RuntimeError(
            f"{ENABLE_GPU_ENV}={os.environ.get(ENABLE_GPU_ENV)!r} selects the reference's NumPy backend, which "
            "spectral_connectivity_amd does not have: every computation here runs on the HIP engine. Unset the "
            "variable or set it to 'true' (or use the reference package for a CPU run).")
    from . import _hosts
    if _hosts.kind() == "numpy":
        # the torch-free host: the library's own device count (the check numpy_host.NumpyHost makes)
        n = c_int(0)
        load(torch_host=False).sc_device_count(byref(n))
        if n.value < 1:
            raise RuntimeError("spectral_connectivity_amd: no ROCm GPU is visible (sc_device_count() = 0). "
                               "This engine has no CPU fallback; run on an MI355X host.")
        return
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(
            "spectral_connectivity_amd: no ROCm GPU is visible (torch.cuda.is_available() is False). "
            "This engine has no CPU fallback; run on an MI355X host.")
    load()


def timing_enable(on=True):
    """Library-side stage timers (hipEvents on the launch stream, sc_timing.hip)."""
    check(_handle().sc_timing_enable(int(bool(on))), "sc_timing_enable")


def last_timing(max_entries=4096):
    """[(entry point, milliseconds)] of the calls since the previous read, in call order (waits for them)."""
    buf = (Timing * max_entries)()
    n = c_int(0)
    check(_handle().sc_last_timing(buf, max_entries, byref(n)), "sc_last_timing")
    return [(buf[i].name.decode(), float(buf[i].ms)) for i in range(n.value)]


# ---- planes format (sc_fused2.hip): when stage A writes it -- shared by the PyTorch host (engine.py) and the NumPy host ----------
PLANES_FORMAT_FAMILIES = (PLANE_CSM, PLANE_CSM | PLANE_ABS_IM, PLANE_CSM | PLANE_ABS_IM | PLANE_IM_SQ,
                          PLANE_SIGN_IM)   # what sc_fused2.hip accumulates


PLANES_FORMAT_MIN_CHANNELS = 44
PLANES_FORMAT_MAX_CHANNELS = 1024      # F2_MAX_SIGNALS of csrc/sc_fused2.hip
PLANES_MIN_TYPICAL = 2.5       # SC_PLANES_MIN_TYPICAL of include/sc_hip.h: smallest typical coefficient (scaled units) the format is used for


def padded_channels(n_signals, limit):
    """Channels per row of the float32 engine's spectra: an odd count gets ONE all-zero channel (16-byte aligned rows, even counts for
    the one-pass stage-B kernels) while that stays within the caller's ``limit`` (PLANES_FORMAT_MAX_CHANNELS, or 256: complex64 only)."""
    return n_signals + 1 if (n_signals % 2 and n_signals + 1 <= limit) else n_signals


def planes_format_applies(n_window, n_fft, n_alloc, planes_hint, spectra_bytes=None):
    """Does stage A write the planes format for a caller that will ask for the accumulator families ``planes_hint``?
    ``spectra_bytes``: size of the complex64 spectra of the request, when the caller knows it.

    Round 5: for every family sc_fused2.hip accumulates the answer depends on the SHAPE of the request alone -- not on which of
    those families is asked for first -- so that a ``Connectivity`` takes the same kernels whatever the order of the calls (the
    reference computes every measure from the same coefficients, connectivity.py:463-526).  The format is taken from 44 signals on
    (where CSM + |Im s|, the BASELINE pair coherence + wPLI, first wins: profiles/r04_shape_sweep.txt; at 44 ... 60 signals the
    (Im s)^2 pass alone would be 0.7 ms faster on complex64, at 130 signals CSM alone 0.7 ms -- the price of one path) for requests
    of at least 256 MB of spectra (a few tens of MB are three short launches either way and the scale pass would only add two).
    Families outside the format (the unit-phasor plane of PLV / PPC) and callers without a hint (Granger, canonical and global
    coherence: CSM of every bin, window lengths beyond the format) keep complex64."""
    if planes_hint not in PLANES_FORMAT_FAMILIES or os.environ.get("SC_PLANES_FORMAT", "1") == "0":
        return False
    lo = PLANES_FORMAT_MIN_CHANNELS
    forced = os.environ.get("SC_PLANES_MIN_CHANNELS")               # (tests: the format from this many channels on, whatever the size)
    if forced is not None:
        lo = int(forced)
    elif spectra_bytes is not None and spectra_bytes < (256 << 20):
        return False
    # (up to 1024 signals since round 6: sc_fused2.hip plans its launches over any number of 32-channel blocks; 256 before)
    return lo <= n_alloc <= PLANES_FORMAT_MAX_CHANNELS and bool(_handle().sc_multitaper_fft_planes_supported(n_window, n_fft, n_alloc))
