"""ctypes binding of libdvbs2_fec_hip.so (include/dvbs2_fec_hip.h).

This is the stub a maintainer of the reference would bind (see INTEGRATION.md for the C++ side);
the tests and bench.py drive the C ABI through it. There is deliberately no fallback: if the
shared library is missing, import of this module raises.
"""
import ctypes as C
import os

# One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so (SONAME libamdhip64.so.7) and
# resolves it by file name, so it must be loaded BEFORE this library, whose NEEDED libamdhip64.so.7
# then binds to the already-loaded copy. Loading in the other order puts two HIP/HSA runtimes in the
# process and the second one finds no GPU. torch is plumbing here (device buffers, streams, RCCL).
try:
    import torch  # noqa: F401
except ImportError:  # standalone use (e.g. from the GNU Radio blocks): the system ROCm runtime is used
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVBS2_LIB") or os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libdvbs2_fec_hip.so"))  # DVBS2_LIB: kernel experiments

OK, EINVAL, EDEVICE, ESIZE = 0, -1, -2, -3
STANDARD_DVBS2, STANDARD_DVBT2 = 0, 1
FECFRAME_SHORT, FECFRAME_NORMAL, FECFRAME_MEDIUM = 0, 1, 2
OM_CODEWORD, OM_MESSAGE = 0, 1
MOD_QPSK, MOD_8PSK, MOD_16APSK, MOD_32APSK = 0, 4, 6, 8
ENC_NO_MAPPER = -1
PULSE_TILE = 512  # DVBS2_PULSE_TILE: symbols per workgroup of the pulse shaper's kernel
RESAMP_TILE = 1024  # DVBS2_RESAMP_TILE: output samples per workgroup of the resampler's kernel
DDC_SPAN, DDC_MAX_TILE = 9216, 1024  # DVBS2_DDC_SPAN, DVBS2_DDC_MAX_TILE: a workgroup of the down-converter's kernel stages at most DDC_SPAN
# mixed samples and writes min(DDC_MAX_TILE, (DDC_SPAN - (ntaps - 1)) // decim) output samples
PFBCH_SPAN, PFBCH_MAX_TILE = 5376, 1024  # DVBS2_PFBCH_SPAN, DVBS2_PFBCH_MAX_TILE: a workgroup of the channelizer's kernel writes
# min(PFBCH_MAX_TILE, (PFBCH_SPAN - (ntaps - 1) - n_chan) // decim) output instants
PFBSYN_SPAN, PFBSYN_SPAN_LONG, PFBSYN_MAX_TILE, PFBSYN_MAX_PRODUCT = 6144, 13312, 512, 8192  # DVBS2_PFBSYN_*: the synthesizer's tile rule
# (dvbs2_pfbsyn_tile) and the largest n_chan * ceil(ntaps / interp) that creation accepts
SPECTRUM_CHUNK = 16  # DVBS2_SPECTRUM_CHUNK: segments whose powers one workgroup of the spectrum kernel adds in order
SPECTRUM_RECT, SPECTRUM_HANN, SPECTRUM_HAMMING, SPECTRUM_BLACKMAN_HARRIS = 0, 1, 2, 3  # DVBS2_SPECTRUM_*: the windows
AGC_TILE = 64  # DVBS2_AGC_TILE: samples per stream and tile of the AGC's kernel
AWGN_TILE = 512  # DVBS2_AWGN_TILE: samples of a row per workgroup of the AWGN channel's kernel
IQ_U8, IQ_S8, IQ_S16 = 0, 1, 2  # DVBS2_IQ_*: the code formats of the IQ sample converter
IQCONV_TILE = 8192  # DVBS2_IQCONV_TILE: samples of a row per workgroup of the IQ sample converter's kernels


class FecInfo(C.Structure):
    _fields_ = [("bch_k", C.c_uint32), ("bch_n", C.c_uint32), ("bch_t", C.c_uint32),
                ("ldpc_k", C.c_uint32), ("ldpc_n", C.c_uint32), ("table_k", C.c_uint32),
                ("table", C.c_char * 24)]


class BbDeheaderCounters(C.Structure):
    _fields_ = [("packets", C.c_uint64), ("errors", C.c_uint64), ("bbframes", C.c_uint64), ("dropped", C.c_uint64),
                ("gaps", C.c_uint64), ("overruns", C.c_uint64), ("synched", C.c_int32), ("partial_ts_bytes", C.c_int32)]


class BbFramerCounters(C.Structure):
    """dvbs2_bbframer_counters_t"""
    _fields_ = [("packets", C.c_uint64), ("bbframes", C.c_uint64), ("sync_errors", C.c_uint64)]


class PlFrameEstimates(C.Structure):
    """dvbs2_plframe_estimates_t: addresses (device or host, by entry point), 0 = not wanted."""
    _fields_ = [("plsc_decoded", C.c_void_p), ("sof_phase", C.c_void_p), ("plheader_phase", C.c_void_p),
                ("pilot_phase", C.c_void_p), ("fine_foffset", C.c_void_p), ("fine_valid", C.c_void_p)]


class PlSyncFrame(C.Structure):
    """dvbs2_plsync_frame_t; PLSYNC_FRAME_DTYPE below is the same record for numpy."""
    _fields_ = [("sof_index", C.c_int64), ("metric", C.c_float), ("plsc", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class SymSyncState(C.Structure):
    """dvbs2_symsync_state_t"""
    _fields_ = [("vi", C.c_double), ("cnt", C.c_double), ("mu", C.c_double), ("n_read", C.c_int64), ("last_xi_re", C.c_float),
                ("last_xi_im", C.c_float), ("jump", C.c_int32), ("init", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class SpectrumCarrierParams(C.Structure):
    """dvbs2_spectrum_carrier_params_t"""
    _fields_ = [("floor_quantile", C.c_double), ("threshold_db", C.c_double), ("smooth", C.c_int32), ("min_gap", C.c_int32),
                ("min_width", C.c_int32), ("reserved", C.c_int32)]


SPECTRUM_CARRIER_DTYPE = [("centre", "<f8"), ("bandwidth", "<f8"), ("level", "<f8"), ("floor", "<f8"), ("lo_bin", "<i4"), ("hi_bin", "<i4")]  # dvbs2_spectrum_carrier_t
PLSYNC_FRAME_DTYPE = [("sof_index", "<i8"), ("metric", "<f4"), ("plsc", "u1"), ("flags", "u1"), ("reserved", "u1", (2,))]
ROTATOR_STATE_DTYPE = [("phase", "<u8"), ("inc", "<u8"), ("index", "<i8"), ("reserved", "<u8")]  # dvbs2_rotator_state_t
BBDEHEADER_STATE_DTYPE = [("synched", "<i4"), ("partial_ts_bytes", "<i4"), ("packets", "<u8"), ("errors", "<u8"), ("bbframes", "<u8"), ("dropped", "<u8"),
                          ("gaps", "<u8"), ("overruns", "<u8"), ("last_packets", "<i4"), ("reserved", "<i4"), ("partial_pkt", "u1", (188,)),
                          ("padding", "u1", (4,))]  # dvbs2_bbdeheader_state_t
PLSYNC_SEARCHING, PLSYNC_FOUND, PLSYNC_LOCKED = 0, 1, 2
PLSYNC_REAL_PEAK, PLSYNC_FLAG_LOCKED = 1, 2


# every symbol include/dvbs2_fec_hip.h declares: name -> (restype, argtypes)
_vp, _i, _ip = C.c_void_p, C.c_int, C.POINTER(C.c_int)
_f, _fp = C.c_float, C.POINTER(C.c_float)
SYMBOLS = {
    "dvbs2_last_error": (C.c_char_p, []),
    "dvbs2_device_count": (_i, []),
    "dvbs2_host_register": (_i, [_vp, C.c_size_t]),
    "dvbs2_host_unregister": (_i, [_vp]),
    "dvbs2_host_is_page_locked": (_i, [_vp, C.c_size_t]),
    "dvbs2_host_alloc": (_i, [C.POINTER(_vp), C.c_size_t]),
    "dvbs2_host_free": (_i, [_vp]),
    "dvbs2_get_fec_info": (_i, [_i, _i, _i, C.POINTER(FecInfo)]),
    "dvbs2_rate_name": (C.c_char_p, [_i]),
    "dvbs2_rate_from_name": (_i, [C.c_char_p]),
    "dvbs2_ldpc_table_info": (_i, [C.c_char_p, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_ldpc_table_name": (C.c_char_p, [_i]),
    "dvbs2_ldpc_layer_info": (_i, [C.c_char_p, _i, _ip, _vp, _vp, _i]),
    "dvbs2_ldpc_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i]),
    "dvbs2_ldpc_create_table": (_i, [C.POINTER(_vp), C.c_char_p, _i, _i, _i, _i]),
    "dvbs2_ldpc_destroy": (None, [_vp]),
    "dvbs2_ldpc_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_ldpc_decode": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "dvbs2_ldpc_decode_device": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_ldpc_enqueue_device": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_ldpc_finish": (_i, [_vp]),
    "dvbs2_ldpc_profile": (_i, [_vp, _i, C.POINTER(C.c_double), _ip]),
    "dvbs2_ldpc_kernel_name": (C.c_char_p, [_vp]),
    "dvbs2_ldpc_fallback_rounds": (_i, [_vp]),
    "dvbs2_measure_host_copy": (_i, [_i, C.c_size_t, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dvbs2_measure_shader_clock": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dvbs2_debug_cu_slot_table": (_i, [_i, _i, C.POINTER(C.c_ulonglong), _ip]),
    "dvbs2_bch_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_bch_create_raw": (_i, [C.POINTER(_vp), _i, C.c_uint32, _i, _i, _i, _i]),
    "dvbs2_bch_destroy": (None, [_vp]),
    "dvbs2_bch_params": (_i, [_vp, _ip, _ip, _ip]),
    "dvbs2_bch_genpoly": (_i, [_vp, _vp, _i]),
    "dvbs2_bch_decode": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_bch_set_descramble": (_i, [_vp, _i]),
    "dvbs2_bb_descramble_sequence": (_i, [_vp, _i]),
    "dvbs2_bch_decode_device": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "dvbs2_demap_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_demap_table_check": (_i, [_i, _vp, _vp]),
    "dvbs2_demap_create_table": (_i, [C.POINTER(_vp), _i, _i, _vp, _vp, _i, _i]),
    "dvbs2_demap_table": (_i, [_vp, _ip, _vp, _vp]),
    "dvbs2_demap_destroy": (None, [_vp]),
    "dvbs2_demap_params": (_i, [_vp, _ip, _ip, _ip, _ip]),
    "dvbs2_apsk_points": (_i, [_i, _i, _vp]),
    "dvbs2_demap_soft": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "dvbs2_demap_soft_device": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "dvbs2_demap_estimate_snr": (_i, [_vp, _vp, _i, _vp]),
    "dvbs2_demap_estimate_snr_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_demap_refine_snr": (_i, [_vp, _vp, _vp, _i, _vp]),
    "dvbs2_demap_refine_snr_device": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "dvbs2_plpayload_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_plpayload_destroy": (None, [_vp]),
    "dvbs2_plpayload_params": (_i, [_vp, _ip, _ip, _ip]),
    "dvbs2_plpayload_process": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "dvbs2_plpayload_process_device": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dvbs2_pl_scrambling_rn": (_i, [_i, _vp, _i]),
    "dvbs2_plframe_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i]),
    "dvbs2_plframe_destroy": (None, [_vp]),
    "dvbs2_plframe_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_plframe_set_plsc_mode": (_i, [_vp, _i, _i]),
    "dvbs2_plframe_set_expected_pls": (_i, [_vp, _vp, _i]),
    "dvbs2_plframe_estimate": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "dvbs2_plframe_estimate_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_plframe_process": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_plframe_process_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "dvbs2_plheader_symbols": (_i, [_i, _vp]),
    "dvbs2_pls_parse": (_i, [_i, _ip, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_plsync_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_plsync_destroy": (None, [_vp]),
    "dvbs2_plsync_reset": (_i, [_vp]),
    "dvbs2_plsync_set_plsc_mode": (_i, [_vp, _i, _i]),
    "dvbs2_plsync_set_expected_pls": (_i, [_vp, _vp, _i]),
    "dvbs2_plsync_metric_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_plsync_search_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_plsync_finish": (_i, [_vp, _ip, _ip, _ip]),
    "dvbs2_plsync_search": (_i, [_vp, _vp, _i, _vp, _ip, _ip, _ip]),
    "dvbs2_plsync_gather_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "dvbs2_plsync_taps": (_i, [_vp, _vp]),
    "dvbs2_plsync_thresholds": (_i, [_vp, _vp]),
    "dvbs2_plcoarse_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i]),
    "dvbs2_plcoarse_destroy": (None, [_vp]),
    "dvbs2_plcoarse_reset": (_i, [_vp]),
    "dvbs2_plcoarse_estimate_device": (_i, [_vp, _vp, C.c_int64, _vp, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_plcoarse_estimate_records_device": (_i, [_vp, _vp, _i, C.c_int64, _vp, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_plcoarse_estimate": (_i, [_vp, _vp, C.c_int64, _vp, _i, _vp, _vp, _vp]),
    "dvbs2_plcoarse_weights": (_i, [_i, _vp]),
    "dvbs2_agc_check": (_i, [_f, _f, _f, _f]),
    "dvbs2_agc_create": (_i, [C.POINTER(_vp), _f, _f, _f, _f, _i, _i, _i]),
    "dvbs2_agc_destroy": (None, [_vp]),
    "dvbs2_agc_reset": (_i, [_vp]),
    "dvbs2_agc_set_params": (_i, [_vp, _f, _f, _f]),
    "dvbs2_agc_set_swap_iq": (_i, [_vp, _i]),
    "dvbs2_agc_set_gain": (_i, [_vp, _i, _f]),
    "dvbs2_agc_params": (_i, [_vp, _fp, _fp, _fp, _ip, _ip]),
    "dvbs2_agc_state": (_i, [_vp, _vp, _i]),
    "dvbs2_agc_work_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "dvbs2_agc_work": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_awgn_sigma": (_i, [C.c_double, C.c_double, _i, _fp]),
    "dvbs2_awgn_words": (_i, [C.c_uint64, C.c_uint64, C.c_int64, _vp]),
    "dvbs2_awgn_sample": (_i, [C.c_uint64, C.c_uint64, C.c_int64, _vp]),
    "dvbs2_awgn_check": (_i, [_f, _i, _i]),
    "dvbs2_awgn_create": (_i, [C.POINTER(_vp), C.c_uint64, _f, _i, _i, _i]),
    "dvbs2_awgn_destroy": (None, [_vp]),
    "dvbs2_awgn_set_sigma": (_i, [_vp, _f]),
    "dvbs2_awgn_set_seed": (_i, [_vp, C.c_uint64]),
    "dvbs2_awgn_params": (_i, [_vp, C.POINTER(C.c_uint64), _fp, _ip, _ip]),
    "dvbs2_awgn_add_device": (_i, [_vp, _vp, C.c_int64, _i, _i, C.c_uint64, C.c_int64, _vp, _vp, C.c_int64, _vp]),
    "dvbs2_awgn_add": (_i, [_vp, _vp, _i, C.c_uint64, C.c_int64, _vp]),
    "dvbs2_iqconv_bytes": (_i, [_i]),
    "dvbs2_iqconv_check": (_i, [_i, _f, _i, _i]),
    "dvbs2_iqconv_unpack_host": (_i, [_i, _f, _vp, C.c_int64, _vp, _vp]),
    "dvbs2_iqconv_pack_host": (_i, [_i, _f, _vp, C.c_int64, _vp, _vp]),
    "dvbs2_iqconv_create": (_i, [C.POINTER(_vp), _i, _f, _i, _i, _i]),
    "dvbs2_iqconv_destroy": (None, [_vp]),
    "dvbs2_iqconv_set_gain": (_i, [_vp, _f]),
    "dvbs2_iqconv_params": (_i, [_vp, _ip, _fp, _ip, _ip, _ip]),
    "dvbs2_iqconv_unpack_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _vp, _vp]),
    "dvbs2_iqconv_pack_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _vp, _vp]),
    "dvbs2_iqconv_unpack_to_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_iqconv_pack_from_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_rotator_create": (_i, [C.POINTER(_vp), C.c_double, _i]),
    "dvbs2_rotator_destroy": (None, [_vp]),
    "dvbs2_rotator_reset": (_i, [_vp]),
    "dvbs2_rotator_set_phase_inc": (_i, [_vp, C.c_double]),
    "dvbs2_rotator_schedule": (_i, [_vp, C.c_int64, C.c_double]),
    "dvbs2_rotator_seek": (_i, [_vp, C.c_int64]),
    "dvbs2_rotator_position": (_i, [_vp, C.POINTER(C.c_int64), _ip]),
    "dvbs2_rotator_rotate_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_rotator_rotate": (_i, [_vp, _vp, _i, _vp]),
    "dvbs2_rotator_measure": (_i, [_i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # rotator rows: state in the caller's device memory, no handle
    "dvbs2_rotator_state_init": (_i, [_vp, _i, _vp]),
    "dvbs2_rotator_state_read": (_i, [_vp, _i, _vp, _vp]),
    "dvbs2_rotator_adjust_turns": (_i, [_f, C.c_double, C.POINTER(C.c_int64), _ip]),
    "dvbs2_rotator_rows_check": (_i, [C.c_int64, C.c_int64, _i, _i, C.c_int64]),
    "dvbs2_rotator_rows_device": (_i, [_vp, C.c_int64, _vp, C.c_int64, _i, _i, C.c_int64, _vp, _i, _vp]),
    "dvbs2_rotator_retune_device": (_i, [_vp, _i, C.c_int64, C.c_double, _i, _vp]),
    "dvbs2_rotator_control_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int64, _vp, _vp, _vp, _i, _vp]),
    "dvbs2_symsync_loop_constants": (_i, [_i, _f, _f, _f, _fp, _fp, _fp]),
    "dvbs2_symsync_geometry": (_i, [_i, _i, _i, _i, _ip, _ip, _ip]),
    "dvbs2_symsync_taps": (_i, [_i, _f, _i, _i, _vp]),
    "dvbs2_symsync_create": (_i, [C.POINTER(_vp), _i, _f, _f, _f, _i, _i, _i, _i, _i, _i]),
    "dvbs2_symsync_create_taps": (_i, [C.POINTER(_vp), _i, _f, _f, _f, _i, _i, _i, _vp, _i, _i, _i]),
    "dvbs2_symsync_destroy": (None, [_vp]),
    "dvbs2_symsync_reset": (_i, [_vp]),
    "dvbs2_symsync_params": (_i, [_vp, _ip, _ip, _ip, _fp, _fp, _fp]),
    "dvbs2_symsync_work_device": (_i, [_vp, _vp, C.c_int64, _vp, _i, _vp, C.c_int64, _i, _vp, _vp, _vp]),
    "dvbs2_symsync_finish": (_i, [_vp, _vp, _vp, _vp]),
    "dvbs2_symsync_state": (_i, [_vp, _i, C.POINTER(SymSyncState)]),
    "dvbs2_symsync_work": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _ip, _ip, _ip]),
    "dvbs2_pulse_geometry": (_i, [_i, _i, _ip, _ip, _ip]),
    "dvbs2_pulse_taps": (_i, [_i, _f, _i, C.c_double, C.c_double, _vp]),
    "dvbs2_pulse_scale_taps": (_i, [_vp, _i, _i, C.c_double]),
    "dvbs2_pulse_create": (_i, [C.POINTER(_vp), _i, _f, _i, _i, _i, _i]),
    "dvbs2_pulse_create_taps": (_i, [C.POINTER(_vp), _i, _vp, _i, _i, _i, _i]),
    "dvbs2_pulse_destroy": (None, [_vp]),
    "dvbs2_pulse_reset": (_i, [_vp]),
    "dvbs2_pulse_params": (_i, [_vp, _ip, _ip, _ip, _ip]),
    "dvbs2_pulse_shape_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _vp]),
    "dvbs2_pulse_shape": (_i, [_vp, _vp, _i, _vp]),
    "dvbs2_resamp_step": (_i, [C.c_double, C.POINTER(C.c_uint64)]),
    "dvbs2_resamp_geometry": (_i, [_i, _i, _ip, _ip, _ip]),
    "dvbs2_resamp_max_out": (C.c_int64, [C.c_uint64, _i]),
    "dvbs2_resamp_check": (_i, [_i, _vp, _i, C.c_double, _i, _i]),
    "dvbs2_resamp_create": (_i, [C.POINTER(_vp), _i, _vp, _i, C.c_double, _i, _i, _i]),
    "dvbs2_resamp_destroy": (None, [_vp]),
    "dvbs2_resamp_reset": (_i, [_vp]),
    "dvbs2_resamp_reset_phase": (_i, [_vp, _vp]),
    "dvbs2_resamp_set_rate": (_i, [_vp, C.c_double]),
    "dvbs2_resamp_set_step": (_i, [_vp, C.c_uint64]),
    "dvbs2_resamp_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip, C.POINTER(C.c_uint64)]),
    "dvbs2_resamp_produce": (_i, [_vp, _i, _i, _vp]),
    "dvbs2_resamp_state": (_i, [_vp, _vp]),
    "dvbs2_resamp_process_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _vp, _vp]),
    "dvbs2_resamp_process": (_i, [_vp, _vp, _i, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "dvbs2_ddc_geometry": (_i, [_i, _i, _ip, _ip]),
    "dvbs2_ddc_produce": (C.c_int64, [C.c_int64, _i, _i]),
    "dvbs2_ddc_check": (_i, [_i, _vp, _i, _i, _i, _i]),
    "dvbs2_ddc_create": (_i, [C.POINTER(_vp), _i, _vp, _i, _i, _i, _i, _i]),
    "dvbs2_ddc_destroy": (None, [_vp]),
    "dvbs2_ddc_reset": (_i, [_vp]),
    "dvbs2_ddc_set_channel": (_i, [_vp, _i, _i, C.c_double]),
    "dvbs2_ddc_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_ddc_position": (_i, [_vp, C.POINTER(C.c_int64)]),
    "dvbs2_ddc_channel": (_i, [_vp, _i, _ip, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "dvbs2_ddc_state": (_i, [_vp, _vp]),
    "dvbs2_ddc_process_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64), _vp]),
    "dvbs2_ddc_process": (_i, [_vp, _vp, C.c_int64, _i, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "dvbs2_spectrum_geometry": (_i, [_i, _i, _i, _i, _ip, _ip, _ip]),
    "dvbs2_spectrum_window": (_i, [_i, _i, _vp]),
    "dvbs2_spectrum_twiddles": (_i, [_i, _vp]),
    "dvbs2_spectrum_check": (_i, [_i, _i, _i, _vp, _i, _i]),
    "dvbs2_spectrum_carriers": (_i, [_vp, _i, _i, _vp, _vp, _i, _ip]),
    "dvbs2_spectrum_create": (_i, [C.POINTER(_vp), _i, _i, _i, _vp, _i, _i, _i, _i]),
    "dvbs2_spectrum_destroy": (None, [_vp]),
    "dvbs2_spectrum_params": (_i, [_vp, _ip, _ip, _ip, _ip, C.POINTER(C.c_double)]),
    "dvbs2_spectrum_process_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _ip, _vp]),
    "dvbs2_spectrum_process": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, _ip]),
    "dvbs2_pfbch_geometry": (_i, [_i, _i, _i, _ip, _ip, _ip]),
    "dvbs2_pfbch_produce": (C.c_int64, [C.c_int64, _i, _i]),
    "dvbs2_pfbch_twiddles": (_i, [_i, _vp]),
    "dvbs2_pfbch_check": (_i, [_i, _i, _vp, _i, _i, _i]),
    "dvbs2_pfbch_create": (_i, [C.POINTER(_vp), _i, _i, _vp, _i, _i, _i, _i]),
    "dvbs2_pfbch_destroy": (None, [_vp]),
    "dvbs2_pfbch_reset": (_i, [_vp]),
    "dvbs2_pfbch_set_channels": (_i, [_vp, _vp, _i]),
    "dvbs2_pfbch_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_pfbch_position": (_i, [_vp, C.POINTER(C.c_int64)]),
    "dvbs2_pfbch_channels": (_i, [_vp, _vp, _ip]),
    "dvbs2_pfbch_process_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64), _vp]),
    "dvbs2_pfbch_process": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "dvbs2_pfbsyn_geometry": (_i, [_i, _i, _i, _ip, _ip, _ip]),
    "dvbs2_pfbsyn_tile": (_i, [_i, _i, _i]),
    "dvbs2_pfbsyn_check": (_i, [_i, _i, _vp, _i, _i, _i]),
    "dvbs2_pfbsyn_create": (_i, [C.POINTER(_vp), _i, _i, _vp, _i, _i, _i, _i]),
    "dvbs2_pfbsyn_destroy": (None, [_vp]),
    "dvbs2_pfbsyn_reset": (_i, [_vp]),
    "dvbs2_pfbsyn_set_channels": (_i, [_vp, _vp, _i]),
    "dvbs2_pfbsyn_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_pfbsyn_position": (_i, [_vp, C.POINTER(C.c_int64)]),
    "dvbs2_pfbsyn_channels": (_i, [_vp, _vp, _ip]),
    "dvbs2_pfbsyn_process_device": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64), _vp]),
    "dvbs2_pfbsyn_process": (_i, [_vp, _vp, C.c_int64, _i, _i, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "dvbs2_bbdeheader_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_bbdeheader_create_raw": (_i, [C.POINTER(_vp), _i, _i, _i]),
    "dvbs2_bbdeheader_destroy": (None, [_vp]),
    "dvbs2_bbdeheader_params": (_i, [_vp, _ip, _ip, _ip]),
    "dvbs2_bbdeheader_process": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int64)]),
    "dvbs2_bbdeheader_process_device": (_i, [_vp, _vp, _i, _vp, _vp]),
    "dvbs2_bbdeheader_finish": (_i, [_vp, C.POINTER(C.c_int64), _vp]),
    "dvbs2_bbdeheader_counters": (_i, [_vp, _vp, _vp]),
    "dvbs2_bbdeheader_reset": (_i, [_vp, _vp]),
    # de-header rows: state in the caller's device memory, no handle
    "dvbs2_bbdeheader_rows_check": (_i, [_i, _i, _i]),
    "dvbs2_bbdeheader_rows_geometry": (_i, [_i, _i, _i, _ip, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dvbs2_bbdeheader_state_counters": (_i, [_vp, _i, _vp]),
    "dvbs2_bbdeheader_rows_device": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _i, _vp]),
    "dvbs2_bbframer_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_bbframer_create_raw": (_i, [C.POINTER(_vp), _i, _i, _i]),
    "dvbs2_bbframer_destroy": (None, [_vp]),
    "dvbs2_bbframer_params": (_i, [_vp, _ip, _ip, _ip]),
    "dvbs2_bbframer_set_matype": (_i, [_vp, _i, _i]),
    "dvbs2_bbframer_need": (_i, [_vp, _i, _i, _ip]),
    "dvbs2_bbframer_process_device": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "dvbs2_bbframer_process": (_i, [_vp, _vp, _i, _i, _vp, _ip]),
    "dvbs2_bbframer_counters": (_i, [_vp, _vp, _vp]),
    "dvbs2_bbframer_reset": (_i, [_vp, _vp]),
    "dvbs2_bbheader_build": (_i, [_vp, _i, _i, _i, _i, _i, _i]),
    "dvbs2_crc8": (_i, [_vp, C.c_size_t]),
    "dvbs2_chain_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i, _i]),
    "dvbs2_chain_create_table": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _vp, _vp, _i, _i, _i]),
    "dvbs2_chain_destroy": (None, [_vp]),
    "dvbs2_chain_params": (_i, [_vp, _ip, _ip]),
    "dvbs2_chain_set_descramble": (_i, [_vp, _i]),
    "dvbs2_chain_decode_device": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_chain_create_llr": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i]),
    "dvbs2_chain_llr_params": (_i, [_vp, _ip, _ip, _ip]),
    "dvbs2_chain_decode_llr_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_chain_enqueue_device": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_chain_enqueue_llr_device": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_chain_finish": (_i, [_vp]),
    "dvbs2_chain_decode": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "dvbs2_chain_decode_llr": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "dvbs2_chain_ldpc_profile": (_i, [_vp, _i, C.POINTER(C.c_double), _ip]),
    "dvbs2_chain_ldpc_kernel_name": (C.c_char_p, [_vp]),
    "dvbs2_chain_ldpc_fallback_rounds": (_i, [_vp]),
    "dvbs2_enc_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i]),
    "dvbs2_enc_create_table": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _vp, _vp, _i, _i]),
    "dvbs2_enc_create_parts": (_i, [C.POINTER(_vp), _i, C.c_uint32, _i, _i, C.c_char_p, _i, _i]),
    "dvbs2_enc_destroy": (None, [_vp]),
    "dvbs2_enc_params": (_i, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "dvbs2_enc_set_scramble": (_i, [_vp, _i]),
    "dvbs2_enc_check": (_i, [_i, _i, _i, _i]),
    "dvbs2_enc_encode_device": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_enc_encode": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "dvbs2_plframer_layout": (_i, [_vp, _i, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dvbs2_plframer_create": (_i, [C.POINTER(_vp), _i, _i, _i]),
    "dvbs2_plframer_destroy": (None, [_vp]),
    "dvbs2_plframer_set_sequence": (_i, [_vp, _vp, _i]),
    "dvbs2_plframer_params": (_i, [_vp, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dvbs2_plframer_frame_device": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "dvbs2_plframer_frame": (_i, [_vp, _vp, _i, _i, _vp]),
    # the batched stages between the symbol synchroniser and the FEC chain
    "dvbs2_plsync_batch_check": (_i, [_i, _i, _i, _i, _i]),
    "dvbs2_plsync_batch_check_search": (_i, [_i, _i, C.c_int64, _vp, _vp, _i]),
    "dvbs2_plsync_batch_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _i]),
    "dvbs2_plsync_batch_destroy": (None, [_vp]),
    "dvbs2_plsync_batch_reset": (_i, [_vp]),
    "dvbs2_plsync_batch_reset_stream": (_i, [_vp, _i]),
    "dvbs2_plsync_batch_set_plsc_mode": (_i, [_vp, _i, _i]),
    "dvbs2_plsync_batch_set_expected_pls": (_i, [_vp, _vp, _i]),
    "dvbs2_plsync_batch_search_device": (_i, [_vp, _vp, C.c_int64, _vp, _vp, _i, _vp, _vp]),
    "dvbs2_plsync_batch_finish": (_i, [_vp, _vp, _vp, _vp]),
    "dvbs2_plsync_batch_gather_device": (_i, [_vp, _vp, C.c_int64, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "dvbs2_plframe_stride_check": (_i, [_i, C.c_int64]),
    "dvbs2_plframe_estimate_strided_device": (_i, [_vp, _vp, C.c_int64, _i, _vp, _vp, _vp, _vp]),
    "dvbs2_plframe_process_strided_device": (_i, [_vp, _vp, C.c_int64, _i, _vp, _vp, _vp, _vp, _vp]),
    "dvbs2_plcoarse_batch_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i]),
    "dvbs2_plcoarse_batch_destroy": (None, [_vp]),
    "dvbs2_plcoarse_batch_reset": (_i, [_vp]),
    "dvbs2_plcoarse_batch_reset_stream": (_i, [_vp, _i]),
    "dvbs2_plcoarse_batch_estimate_device": (_i, [_vp, _vp, C.c_int64, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} not found: build it with `make -C gr-dvbs2rx_amd` "
                      "(or __graft_entry__.build()); there is no CPU fallback")
lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in SYMBOLS.items():
    if os.environ.get("DVBS2_LIB") and not hasattr(lib, _name):
        continue  # kernel experiments against a library built from an older tree (tools/ab.sh); the product library must export all
    _fn = getattr(lib, _name)  # (not _f: that is the c_float alias SYMBOLS is written with)
    _fn.restype = _res
    _fn.argtypes = _args


class Dvbs2Error(RuntimeError):
    def __init__(self, code):
        self.code = code
        super().__init__(f"libdvbs2_fec_hip error {code}: {lib.dvbs2_last_error().decode()}")


def check(code):
    if code < 0:
        raise Dvbs2Error(code)
    return code
