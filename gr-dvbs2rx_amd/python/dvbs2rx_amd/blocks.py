"""Python view of the three reference blocks' compute, calling the C ABI.

Names and argument meaning follow the reference block constructors:
  ldpc_decoder_bb.make(standard, framesize, rate, constellation, outputmode, infomode, max_trials, debug_level)
      include/gnuradio/dvbs2rx/ldpc_decoder_bb.h:37-44
The Python classes exist for the tests and the benchmark; the production drop-in is the C++ shim
in INTEGRATION.md that calls the same C entry points from the blocks' general_work().
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import lib, check

__all__ = ["get_fec_info", "rate_id", "LdpcDecoder", "BchDecoder", "Demapper", "FecChain", "BbDeheader", "ldpc_table_info", "ldpc_layer_info",
           "ldpc_table_names", "bb_descramble_sequence", "PlPayload",
           "pl_scrambling_rn", "HostBuffer", "PlFrontEnd", "plheader_symbols", "pls_parse", "apsk_points", "demap_table_check",
           "PlSync", "plsync_taps", "plsync_thresholds", "PlCoarse", "plcoarse_weights", "PlSyncBatch", "PlCoarseBatch", "plsync_batch_check", "Agc", "agc_check", "Awgn", "awgn_sigma", "awgn_words",
           "awgn_sample", "awgn_check", "IqConverter", "IQ_FORMATS", "iqconv_bytes", "iqconv_check", "iqconv_unpack_host", "iqconv_pack_host",
           "Rotator", "ROTATOR_STATE", "rotator_state_init", "rotator_state_read", "rotator_adjust_turns", "rotator_rows_device",
           "rotator_retune_device", "rotator_control_device",
           "SymbolSync", "symsync_loop_constants", "symsync_geometry", "symsync_taps", "FecEncoder", "enc_check",
           "PlFramer", "plframer_layout", "PulseShaper", "pulse_geometry", "pulse_taps", "pulse_scale_taps",
           "Resampler", "resamp_step", "resamp_geometry", "resamp_max_out", "resamp_check",
           "Ddc", "ddc_geometry", "ddc_produce", "ddc_check", "ddc_tile",
           "Spectrum", "spectrum_geometry", "spectrum_window", "spectrum_twiddles", "spectrum_check", "spectrum_carriers",
           "PfbChannelizer", "pfbch_geometry", "pfbch_produce", "pfbch_check", "pfbch_tile", "pfbch_twiddles",
           "PfbSynthesizer", "pfbsyn_geometry", "pfbsyn_check", "pfbsyn_tile",
           "BBDEHEADER_STATE", "bbdeheader_rows_check", "bbdeheader_rows_geometry", "bbdeheader_state_counters", "bbdeheader_rows_device",
           "BbFramer", "bbheader_build", "crc8"]

DEFAULT_TRIALS = 25  # reference lib/ldpc_decoder_bb_impl.cc:391


def _ints(k, entry, *args):
    """The k ints that `entry` writes through its last k pointer arguments."""
    v = [C.c_int() for _ in range(k)]
    check(entry(*args, *v))
    return tuple(x.value for x in v)


def _ptr(a):
    """The address of an array's data; None for an empty array or for None."""
    return a.ctypes.data if a is not None and a.size else None


def _f32_vector(x):
    """(array, pointer, size) of x as a C-contiguous float32 vector: taps and windows. Keep the array while the pointer is in use."""
    v = np.ascontiguousarray(x, np.float32).reshape(-1)
    return v, _ptr(v), int(v.size)


def _complex64(x, name, rows=None):
    """x as a C-contiguous complex64 vector. rows names the matrix form ("[n_inputs, n_in]") where the stage takes one: a vector is then
    one row of it."""
    x = np.asarray(x)
    if x.dtype != np.complex64:
        raise TypeError(f"{name} must be complex64, not {x.dtype}")
    if rows and x.ndim == 1:
        x = x.reshape(1, -1)
    if x.ndim != (2 if rows else 1) or not x.flags.c_contiguous:
        raise ValueError(f"{name} must be a C-contiguous vector" + (f" or {rows} matrix" if rows else ""))
    return x


class _Handle:
    """One C handle: self._h is there (null) before a subclass's constructor runs and creates it; the subclass names the destroy entry.
    close() may be called again, and runs when the object is dropped."""
    _destroy = None

    def __new__(cls, *args, **kwargs):
        self = super().__new__(cls)
        self._h = C.c_void_p()
        return self

    def close(self):
        if self._h:
            self._destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rate_id(rate):
    if isinstance(rate, str):
        r = lib.dvbs2_rate_from_name(rate.encode())
        if r < 0:
            raise ValueError(f"unknown code rate {rate}")
        return r
    return int(rate)


def get_fec_info(standard, framesize, rate):
    fi = capi.FecInfo()
    check(lib.dvbs2_get_fec_info(standard, framesize, rate_id(rate), fi))
    return dict(bch_k=fi.bch_k, bch_n=fi.bch_n, bch_t=fi.bch_t, ldpc_k=fi.ldpc_k, ldpc_n=fi.ldpc_n,
                table_k=fi.table_k, table=fi.table.decode())


def ldpc_table_info(table):
    return dict(zip(("N", "K", "q", "links_total", "conflict_layers"), _ints(5, lib.dvbs2_ldpc_table_info, table.encode())))


def bb_descramble_sequence(n_bytes):
    """The BBFRAME energy-dispersal PRBS as packed bytes (reference lib/bbdescrambler_bb_impl.cc:51-65)."""
    seq = np.zeros(n_bytes, np.uint8)
    check(lib.dvbs2_bb_descramble_sequence(seq.ctypes.data, n_bytes))
    return seq


class HostBuffer:
    """A page-locked host buffer allocated by the driver (dvbs2_host_alloc -> hipHostMalloc) with a numpy view: what a caller of the
    host-pointer entry points should hand over where it can choose its memory (include/dvbs2_fec_hip.h). `array` stays valid until
    free() / the object is dropped."""

    def __init__(self, shape, dtype):
        self.array = None
        self._p = C.c_void_p()
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        check(lib.dvbs2_host_alloc(C.byref(self._p), max(n, 1)))
        self.nbytes = n
        self.array = np.frombuffer((C.c_char * max(n, 1)).from_address(self._p.value), dtype=dt, count=int(np.prod(shape))).reshape(shape)

    @property
    def ptr(self):
        return self._p.value

    def free(self):
        if self._p:
            self.array = None
            lib.dvbs2_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ldpc_table_names():
    """Names of all built-in LDPC tables (the reference's DVB_*_TABLE_* structs)."""
    out, i = [], 0
    while True:
        n = lib.dvbs2_ldpc_table_name(i)
        if n is None:
            return out
        out.append(n.decode())
        i += 1


def ldpc_layer_info(table, layer):
    g = np.zeros(64, np.int32)
    s = np.zeros(64, np.int32)
    blk = C.c_int()
    cnt = check(lib.dvbs2_ldpc_layer_info(table.encode(), layer, blk, g.ctypes.data, s.ctypes.data, 64))
    return dict(cnt=cnt, block=blk.value, groups=g[:cnt].tolist(), shifts=s[:cnt].tolist())


class LdpcDecoder(_Handle):
    """ldpc_decoder_bb's compute: batches of int8 LLR frames -> packed hard bits (+ decoded LLRs)."""
    _destroy = lib.dvbs2_ldpc_destroy

    def __init__(self, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2",
                 outputmode=capi.OM_MESSAGE, max_trials=0, group_size=32, max_frames=64, device=0,
                 table=None, message_bits=None):
        if table is not None:
            check(lib.dvbs2_ldpc_create_table(C.byref(self._h), table.encode(), int(message_bits),
                                              group_size, max_frames, device))
        else:
            check(lib.dvbs2_ldpc_create(C.byref(self._h), standard, framesize, rate_id(rate),
                                        group_size, max_frames, device))
        self.N, self.K, self.message_bits, self.q, self.group_size = _ints(5, lib.dvbs2_ldpc_params, self._h)
        self.outputmode = outputmode
        self.max_trials = DEFAULT_TRIALS if max_trials == 0 else max_trials
        self.max_frames = max_frames
        # counters behind get_average_trials() (reference lib/ldpc_decoder_bb_impl.h:63, .cc:411-419)
        self.total_trials = 0
        self.batch_cnt = 0
        self.frame_cnt = 0

    @property
    def out_bytes(self):
        return (self.message_bits if self.outputmode == capi.OM_MESSAGE else self.N) // 8

    def _account(self, ret):
        for r in ret:
            self.total_trials += self.max_trials if r < 0 else self.max_trials - int(r)
            self.batch_cnt += 1

    def get_average_trials(self):
        return self.total_trials // self.batch_cnt

    def work(self, llr, want_llr=False):
        """llr: (n_frames, N) int8 host array. Returns (bits (n_frames, out_bytes) uint8, llr_out or None, ret per group)."""
        llr = np.ascontiguousarray(llr, dtype=np.int8)
        nf = llr.shape[0]
        assert llr.shape == (nf, self.N)
        bits = np.empty((nf, self.out_bytes), np.uint8)
        out = np.empty((nf, self.N), np.int8) if want_llr else None
        ng = (nf + self.group_size - 1) // self.group_size
        ret = np.empty(ng, np.int32)
        check(lib.dvbs2_ldpc_decode(self._h, llr.ctypes.data, nf, self.max_trials, self.outputmode,
                                    bits.ctypes.data, out.ctypes.data if want_llr else None, ret.ctypes.data))
        self._account(ret)
        self.frame_cnt += nf
        return bits, out, ret

    def work_device(self, d_llr, n_frames, d_bits, d_llr_out=0, d_ret=0, stream=0):
        """Device-pointer variant (ints from torch.Tensor.data_ptr()); stream = raw hipStream_t value."""
        check(lib.dvbs2_ldpc_decode_device(self._h, d_llr, n_frames, self.max_trials, self.outputmode,
                                           d_bits, d_llr_out or None, d_ret or None, stream or None))

    def enqueue_device(self, d_llr, n_frames, d_bits, d_llr_out=0, d_ret=0, stream=0):
        """work_device without the host synchronisation; finish() completes it."""
        check(lib.dvbs2_ldpc_enqueue_device(self._h, d_llr, n_frames, self.max_trials, self.outputmode,
                                            d_bits, d_llr_out or None, d_ret or None, stream or None))

    def finish(self):
        check(lib.dvbs2_ldpc_finish(self._h))

    @property
    def kernel_name(self):
        return lib.dvbs2_ldpc_kernel_name(self._h).decode()

    def profile(self, enable=True):
        ms, n = C.c_double(), C.c_int()
        check(lib.dvbs2_ldpc_profile(self._h, 1 if enable else 0, ms, n))
        return ms.value, n.value

    @property
    def fallback_rounds(self):
        """host-driven resolution rounds of the group stop since creation (zero in normal operation)"""
        return lib.dvbs2_ldpc_fallback_rounds(self._h)


class BchDecoder(_Handle):
    """bch_decoder_bb's compute (reference lib/bch_decoder_bb_impl.cc:84-117): n/8-byte codewords -> k/8-byte messages."""
    _destroy = lib.dvbs2_bch_destroy

    def __init__(self, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2", max_frames=64,
                 device=0, raw=None):
        if raw is not None:
            m, prim, t, n = raw
            check(lib.dvbs2_bch_create_raw(C.byref(self._h), m, prim, t, n, max_frames, device))
        else:
            check(lib.dvbs2_bch_create(C.byref(self._h), standard, framesize, rate_id(rate), max_frames, device))
        self.n, self.k, self.t = _ints(3, lib.dvbs2_bch_params, self._h)
        # counters behind get_frame_count / get_error_count (lib/bch_decoder_bb_impl.h:46-47)
        self.frame_cnt = 0
        self.frame_error_cnt = 0

    def set_descramble(self, enable=True):
        """Fuse bbdescrambler_bb (reference lib/bbdescrambler_bb_impl.cc:67-82) into the output stage."""
        check(lib.dvbs2_bch_set_descramble(self._h, int(bool(enable))))

    def genpoly(self):
        g = np.zeros(256, np.uint8)
        deg = check(lib.dvbs2_bch_genpoly(self._h, g.ctypes.data, 256))
        return g[:deg + 1].copy()

    def work(self, cw):
        cw = np.ascontiguousarray(cw, dtype=np.uint8)
        nf = cw.shape[0]
        assert cw.shape == (nf, self.n // 8)
        msg = np.empty((nf, self.k // 8), np.uint8)
        corr = np.empty(nf, np.int32)
        check(lib.dvbs2_bch_decode(self._h, cw.ctypes.data, nf, msg.ctypes.data, corr.ctypes.data))
        self.frame_cnt += nf
        self.frame_error_cnt += int((corr == -1).sum())
        return msg, corr

    def work_device(self, d_cw, n_frames, d_msg, d_corr, stream=0):
        check(lib.dvbs2_bch_decode_device(self._h, d_cw, n_frames, d_msg, d_corr, stream or None))


def _table_args(points, column):
    """(n_mod, points as complex64, column as uint8 or None) for the table entries; the C side judges the values."""
    pts = np.ascontiguousarray(points, np.complex64).reshape(-1)
    n_mod = int(pts.size).bit_length() - 1
    if pts.size < 2 or pts.size != 1 << n_mod:
        raise ValueError(f"points: a power of two of them, got {pts.size}")
    col = None
    if column is not None:
        col = np.ascontiguousarray(column, np.uint8)
        if col.shape != (n_mod,):
            raise ValueError(f"column: {n_mod} entries, got shape {col.shape}")
    return n_mod, pts, col


def demap_table_check(points, column=None):
    """Whether Demapper.from_table / FecChain.from_table take this table (dvbs2_demap_table_check; raises Dvbs2Error with the text
    that names the argument). points: 2^n_mod complex values, entry i = label i; column as for from_table. Host only."""
    n_mod, pts, col = _table_args(points, column)
    check(lib.dvbs2_demap_table_check(n_mod, pts.ctypes.data, col.ctypes.data if col is not None else None))


class Demapper(_Handle):
    """xfecframe_demapper_cb's compute (reference lib/xfecframe_demapper_cb_impl.cc:101-186): QPSK and 8PSK as in the reference,
    and capi.MOD_16APSK / capi.MOD_32APSK at their DVB-S2 rates (exact max-log, natural column order; notes/apsk_demap.md).
    from_table(): the same max-log for a caller's table of 4 .. 256 points (notes/demap_table.md)."""
    _destroy = lib.dvbs2_demap_destroy

    def __init__(self, framesize=capi.FECFRAME_NORMAL, rate="C1_2", constellation=capi.MOD_QPSK, max_frames=64, device=0):
        check(lib.dvbs2_demap_create(C.byref(self._h), framesize, rate_id(rate), constellation, max_frames, device))
        self.n_syms, self.n_llr, self.n_mod, self.column_order = _ints(4, lib.dvbs2_demap_params, self._h)

    @classmethod
    def from_table(cls, framesize, points, column=None, max_frames=64, device=0):
        """points: 2^n_mod complex values (n_mod in 2, 3, 4, 5, 6, 8), entry i = the point with label i, used as given. column[c]: the
        label bit (0 = most significant) whose LLRs fill column c of a frame; None = the natural order. column_order is 0 for the
        natural order and -1 otherwise."""
        n_mod, pts, col = _table_args(points, column)
        self = cls.__new__(cls)
        check(lib.dvbs2_demap_create_table(C.byref(self._h), framesize, n_mod, pts.ctypes.data, col.ctypes.data if col is not None else None,
                                           max_frames, device))
        self.n_syms, self.n_llr, self.n_mod, self.column_order = _ints(4, lib.dvbs2_demap_params, self._h)
        return self

    def table(self):
        """(points complex64, column uint8) as a from_table() handle was given them (dvbs2_demap_table)."""
        pts, col = np.empty(1 << self.n_mod, np.complex64), np.empty(self.n_mod, np.uint8)
        check(lib.dvbs2_demap_table(self._h, None, pts.ctypes.data, col.ctypes.data))
        return pts, col

    def work(self, syms, n0):
        """syms: (n_frames, n_syms) complex (converted to complex64); n0: scalar or (n_frames,) float32 -> (n_frames, n_llr) int8."""
        if np.asarray(syms).dtype.kind != "c":
            raise TypeError(f"symbols must be complex, not {np.asarray(syms).dtype}")
        syms = np.ascontiguousarray(syms, dtype=np.complex64)
        nf = syms.shape[0]
        assert syms.shape == (nf, self.n_syms)
        n0 = np.atleast_1d(np.asarray(n0, np.float32))
        out = np.empty((nf, self.n_llr), np.int8)
        check(lib.dvbs2_demap_soft(self._h, syms.ctypes.data, nf, n0.ctypes.data, len(n0), out.ctypes.data))
        return out

    def estimate_snr(self, syms):
        syms = np.ascontiguousarray(syms, dtype=np.complex64)
        nf = syms.shape[0]
        snr = np.empty(nf, np.float32)
        check(lib.dvbs2_demap_estimate_snr(self._h, syms.ctypes.data, nf, snr.ctypes.data))
        return snr

    def refine_snr(self, syms, ref_llr):
        """Post-decoder linear SNR per frame from the decoded LLRs (handle_llr_pdu, reference :268-307)."""
        syms = np.ascontiguousarray(syms, dtype=np.complex64)
        ref_llr = np.ascontiguousarray(ref_llr, dtype=np.int8)
        nf = syms.shape[0]
        assert ref_llr.shape == (nf, self.n_llr)
        snr = np.empty(nf, np.float32)
        check(lib.dvbs2_demap_refine_snr(self._h, syms.ctypes.data, ref_llr.ctypes.data, nf, snr.ctypes.data))
        return snr

    def work_device(self, d_syms, n_frames, d_n0, n0_count, d_llr, stream=0):
        check(lib.dvbs2_demap_soft_device(self._h, d_syms, n_frames, d_n0, n0_count, d_llr, stream or None))


class PlPayload(_Handle):
    """PLFRAME payload step of the PL synchroniser (reference lib/plsync_cc_impl.cc:644-653, :727-795): descramble,
    drop the pilot blocks, de-rotate; produces the XFECFRAME symbols the demapper consumes."""
    _destroy = lib.dvbs2_plpayload_destroy

    def __init__(self, gold_code=0, n_slots=360, has_pilots=True, max_frames=16, device=0):
        check(lib.dvbs2_plpayload_create(C.byref(self._h), gold_code, n_slots, int(bool(has_pilots)), max_frames, device))
        self.payload_len, self.xfecframe_len, self.n_pilots = _ints(3, lib.dvbs2_plpayload_params, self._h)

    def work(self, payload, plheader_phase, fine_foffset, coarse_corrected, pilot_phase=None):
        """payload: (n_frames, payload_len) complex64; per-frame arrays as in plframe_info_t / pl_freq_sync."""
        payload = np.ascontiguousarray(payload, dtype=np.complex64)
        nf = payload.shape[0]
        assert payload.shape == (nf, self.payload_len)
        hph = np.ascontiguousarray(plheader_phase, np.float32)
        cc = np.ascontiguousarray(coarse_corrected, np.int32)
        inc = np.ascontiguousarray(2.0 * np.pi * np.asarray(fine_foffset, np.float64), np.float32)  # :730-731
        pp = np.ascontiguousarray(pilot_phase if pilot_phase is not None else np.zeros((nf, max(self.n_pilots, 1))), np.float32)
        out = np.empty((nf, self.xfecframe_len), np.complex64)
        check(lib.dvbs2_plpayload_process(self._h, payload.ctypes.data, nf, hph.ctypes.data, inc.ctypes.data, cc.ctypes.data,
                                          pp.ctypes.data, out.ctypes.data))
        return out


def apsk_points(constellation, rate):
    """The 16 (capi.MOD_16APSK) or 32 (capi.MOD_32APSK) points of a DVB-S2 code rate, entry i = label i, Es = 1. Host only."""
    out = np.empty(16 if constellation == capi.MOD_16APSK else 32, np.complex64)
    check(lib.dvbs2_apsk_points(int(constellation), rate_id(rate), out.ctypes.data))
    return out


def plheader_symbols(plsc):
    """The 90 expected PLHEADER symbols of a PLSC (SOF + scrambled RM(64,7) codeword, pi/2 BPSK). Host only."""
    out = np.empty(90, np.complex64)
    check(lib.dvbs2_plheader_symbols(int(plsc), out.ctypes.data))
    return out


def pls_parse(plsc):
    """pls_info_t::parse as data (reference lib/pl_signaling.cc:19-61). Host only."""
    return dict(zip(("plframe_len", "payload_len", "xfecframe_len", "n_slots", "n_pilots", "n_mod"), _ints(6, lib.dvbs2_pls_parse, int(plsc))))


class PlFrontEnd(_Handle):
    """PLFRAME front end: per frame the PLSC of its own header, the SOF / PLHEADER / pilot phases and the fine frequency
    offset (reference lib/plsync_cc_impl.cc:582-590, :634-636, :665-680; lib/pl_freq_sync.cc:201-349), then the payload step
    of PlPayload with those estimates. One object = one gold code and one PLSC (frame geometry)."""
    _destroy = lib.dvbs2_plframe_destroy

    EST = (("plsc_decoded", np.uint8), ("sof_phase", np.float32), ("plheader_phase", np.float32), ("pilot_phase", np.float32),
           ("fine_foffset", np.float32), ("fine_valid", np.int32))

    def __init__(self, gold_code=0, plsc=0, max_frames=16, device=0, coherent=True, soft=True, expected_pls=None):
        check(lib.dvbs2_plframe_create(C.byref(self._h), gold_code, plsc, max_frames, device))
        self.plframe_len, self.payload_len, self.xfecframe_len, self.n_slots, self.n_pilots, self.n_mod = _ints(6, lib.dvbs2_plframe_params, self._h)
        self.plsc, self.max_frames = plsc, max_frames
        self.set_plsc_mode(coherent, soft)
        if expected_pls is not None:
            self.set_expected_pls(expected_pls)

    def set_plsc_mode(self, coherent=True, soft=True):
        check(lib.dvbs2_plframe_set_plsc_mode(self._h, int(bool(coherent)), int(bool(soft))))

    def set_expected_pls(self, plsc_list):
        """The enabled-codeword list, in the given order (empty: all 128)."""
        lst = np.asarray(plsc_list)
        if lst.size and (lst.dtype.kind not in "iu" or lst.min() < 0 or lst.max() > 255):
            raise ValueError("expected_pls: integers in 0..127")
        lst = np.ascontiguousarray(lst, np.uint8)
        check(lib.dvbs2_plframe_set_expected_pls(self._h, _ptr(lst), int(lst.size)))

    def _inputs(self, plframes, coarse_corrected, coarse_foffset, trailing_header):
        x = np.asarray(plframes)
        if x.dtype != np.complex64:
            raise TypeError(f"plframes must be complex64, not {x.dtype}")
        if not x.flags.c_contiguous:
            raise ValueError("plframes must be C-contiguous")
        if x.ndim == 2 and x.shape[1] != self.plframe_len or x.ndim not in (1, 2) or x.size % self.plframe_len:
            raise ValueError(f"plframes: expected whole frames of {self.plframe_len} symbols, got shape {x.shape}")
        nf = x.size // self.plframe_len
        if nf > self.max_frames:
            raise ValueError(f"{nf} frames exceed max_frames = {self.max_frames}")
        if trailing_header is not None:
            t = np.asarray(trailing_header)
            if t.dtype != np.complex64 or t.shape != (90,):
                raise ValueError("trailing_header: 90 complex64 symbols")
            x = np.concatenate([x.reshape(-1), t])
        cc = np.asarray(coarse_corrected)
        if cc.shape != (nf,) or cc.dtype.kind not in "biu":
            raise ValueError(f"coarse_corrected: {nf} integers or booleans")
        cc = np.ascontiguousarray(cc, np.int32)
        cf = None
        if coarse_foffset is not None:
            cf = np.asarray(coarse_foffset)
            if cf.shape != (nf,) or cf.dtype.kind != "f":
                raise ValueError(f"coarse_foffset: {nf} floats")
            cf = np.ascontiguousarray(cf, np.float32)
        elif self.n_pilots == 0:
            raise ValueError("a pilotless front end needs coarse_foffset")
        return x, nf, cc, cf

    def _est_arrays(self, nf):
        arrs = {k: np.empty((nf, self.n_pilots) if k == "pilot_phase" else (nf,), dt) for k, dt in self.EST}
        e = capi.PlFrameEstimates(**{k: _ptr(a) for k, a in arrs.items()})
        return arrs, e

    def estimate(self, plframes, coarse_corrected, coarse_foffset=None, trailing_header=None):
        """HOST buffers: plframes complex64 [n_frames, plframe_len] (or flat). Returns the dict of per-frame estimates."""
        x, nf, cc, cf = self._inputs(plframes, coarse_corrected, coarse_foffset, trailing_header)
        arrs, e = self._est_arrays(nf)
        check(lib.dvbs2_plframe_estimate(self._h, x.ctypes.data, nf, int(trailing_header is not None), cc.ctypes.data,
                                         cf.ctypes.data if cf is not None else None, C.byref(e)))
        return arrs

    def work(self, plframes, coarse_corrected, coarse_foffset=None, trailing_header=None):
        """As estimate(), plus the payload step: returns (xfecframes complex64 [n_frames, xfecframe_len], estimates)."""
        x, nf, cc, cf = self._inputs(plframes, coarse_corrected, coarse_foffset, trailing_header)
        arrs, e = self._est_arrays(nf)
        out = np.empty((nf, self.xfecframe_len), np.complex64)
        check(lib.dvbs2_plframe_process(self._h, x.ctypes.data, nf, int(trailing_header is not None), cc.ctypes.data,
                                        cf.ctypes.data if cf is not None else None, out.ctypes.data, C.byref(e)))
        return out, arrs

    def estimate_strided_device(self, d_slots, stride_syms, n_frames, d_coarse_corrected, d_coarse_foffset=0, stream=0, **d_est):
        """DEVICE addresses, asynchronous on `stream`: the estimates of work_strided_device() without the payload step."""
        self.work_strided_device(d_slots, stride_syms, n_frames, d_coarse_corrected, d_coarse_foffset, 0, stream, **d_est)

    def work_strided_device(self, d_slots, stride_syms, n_frames, d_coarse_corrected, d_coarse_foffset=0, d_xfecframes=0, stream=0, **d_est):
        """DEVICE addresses, asynchronous on `stream`: frame f in a slot of its own at symbol f * stride_syms, followed there by its
        next header (stride_syms >= plframe_len + 90; what PlSyncBatch.gather_device writes). d_xfecframes = 0: estimates only."""
        e = capi.PlFrameEstimates(**{k: (v or None) for k, v in d_est.items()})
        if d_xfecframes:
            check(lib.dvbs2_plframe_process_strided_device(self._h, d_slots, int(stride_syms), int(n_frames), d_coarse_corrected,
                                                           d_coarse_foffset or None, d_xfecframes, C.byref(e), stream or None))
        else:
            check(lib.dvbs2_plframe_estimate_strided_device(self._h, d_slots, int(stride_syms), int(n_frames), d_coarse_corrected,
                                                            d_coarse_foffset or None, C.byref(e), stream or None))

    def work_device(self, d_plframes, n_frames, has_trailing_header, d_coarse_corrected, d_coarse_foffset=0, d_xfecframes=0,
                    stream=0, **d_est):
        """DEVICE addresses, asynchronous on `stream`; d_xfecframes = 0: estimates only. d_est: addresses by field name."""
        e = capi.PlFrameEstimates(**{k: (v or None) for k, v in d_est.items()})
        if d_xfecframes:
            check(lib.dvbs2_plframe_process_device(self._h, d_plframes, n_frames, int(has_trailing_header), d_coarse_corrected,
                                                   d_coarse_foffset or None, d_xfecframes, C.byref(e), stream or None))
        else:
            check(lib.dvbs2_plframe_estimate_device(self._h, d_plframes, n_frames, int(has_trailing_header), d_coarse_corrected,
                                                    d_coarse_foffset or None, C.byref(e), stream or None))


class PlSync(_Handle):
    """PLFRAME search on a raw symbol stream (reference lib/pl_frame_sync.cc:66-243): the timing metric for every symbol, the
    searching / found / locked state machine with PLSC decoding at every header, and the gather step that lays the locked
    frames of one PLSC out the way PlFrontEnd reads them. The handle keeps the machine's state and the 89 symbols before the
    consumed point between calls; present the stream again from `consumed`, as with GNU Radio's consume()."""
    _destroy = lib.dvbs2_plsync_destroy

    FRAME_DTYPE = np.dtype(capi.PLSYNC_FRAME_DTYPE)
    MIN_SYMBOLS = 33282 + 90

    def __init__(self, plsc=-1, unlock_thresh=3, max_symbols=1 << 20, max_frames=1024, device=0, coherent=True, soft=True,
                 expected_pls=None):
        """plsc = -1: decode the PLSC of every header; 0..127: the fixed-PLSC (CCM/SIS) mode."""
        check(lib.dvbs2_plsync_create(C.byref(self._h), int(plsc), int(unlock_thresh), int(max_symbols), int(max_frames), device))
        self.plsc, self.unlock_thresh, self.max_symbols, self.max_frames = plsc, unlock_thresh, max_symbols, max_frames
        self.set_plsc_mode(coherent, soft)
        if expected_pls is not None:
            self.set_expected_pls(expected_pls)

    def reset(self):
        check(lib.dvbs2_plsync_reset(self._h))

    def set_plsc_mode(self, coherent=True, soft=True):
        check(lib.dvbs2_plsync_set_plsc_mode(self._h, int(bool(coherent)), int(bool(soft))))

    def set_expected_pls(self, plsc_list):
        """The enabled-codeword list, in the given order (empty: all 128)."""
        lst = np.asarray(plsc_list)
        if lst.size and (lst.dtype.kind not in "iu" or lst.min() < 0 or lst.max() > 127):
            raise ValueError("expected_pls: integers in 0..127")
        lst = np.ascontiguousarray(lst, np.uint8)
        check(lib.dvbs2_plsync_set_expected_pls(self._h, _ptr(lst), int(lst.size)))

    def metric_device(self, d_syms, n_syms, d_metric, stream=0):
        """DEVICE addresses; the timing metric of every index with the handle's history. Does not advance the handle."""
        check(lib.dvbs2_plsync_metric_device(self._h, d_syms, n_syms, d_metric, stream or None))

    def work_device(self, d_syms, n_syms, d_frames, stream=0):
        """DEVICE addresses, asynchronous on `stream`; d_frames: max_frames records of FRAME_DTYPE. Read the result with finish()."""
        check(lib.dvbs2_plsync_search_device(self._h, d_syms, n_syms, d_frames, stream or None))

    def finish(self):
        """Waits for the last work_device(); returns (n_frames, consumed, state)."""
        return _ints(3, lib.dvbs2_plsync_finish, self._h)

    def work(self, syms):
        """HOST buffer of complex64 symbols. Returns (frames as a FRAME_DTYPE array, consumed, state)."""
        x = _complex64(syms, "syms")
        if x.size > self.max_symbols:
            raise ValueError(f"{x.size} symbols exceed max_symbols = {self.max_symbols}")
        frames = np.zeros(self.max_frames, self.FRAME_DTYPE)
        nf, consumed, state = _ints(3, lib.dvbs2_plsync_search, self._h, _ptr(x), int(x.size), frames.ctypes.data)
        return frames[:nf].copy(), consumed, state

    def gather_device(self, d_syms, d_frames, n_frames, wanted_plsc, d_plframes, d_count, stream=0):
        """DEVICE addresses: the locked frames of wanted_plsc among the first n_frames records of the LAST work_device(), back
        to back, then the 90 symbols after the last one (PlFrontEnd's layout with a trailing header); *d_count = frames."""
        check(lib.dvbs2_plsync_gather_device(self._h, d_syms, d_frames, int(n_frames), int(wanted_plsc), d_plframes, d_count, stream or None))


def plsync_taps():
    """Imaginary parts (+-1) of the 25 SOF taps and the 32 PLSC taps of the timing metric, in header order. Host only."""
    sof, pl = np.empty(25, np.float32), np.empty(32, np.float32)
    check(lib.dvbs2_plsync_taps(sof.ctypes.data, pl.ctypes.data))
    return sof, pl


def plsync_thresholds():
    """(unlocked, locked) timing-metric thresholds (reference lib/pl_frame_sync.h:160-162). Host only."""
    u, lk = C.c_float(), C.c_float()
    check(lib.dvbs2_plsync_thresholds(C.byref(u), C.byref(lk)))
    return u.value, lk.value


def plcoarse_weights(full=True):
    """The weighting window of the coarse estimate (reference lib/pl_freq_sync.cc:74-85) as float32: 89 values for the full
    PLHEADER, 25 for the SOF. Host only."""
    w = np.empty(89, np.float32)
    n = check(lib.dvbs2_plcoarse_weights(int(bool(full)), w.ctypes.data))
    return w[:n].copy()


class PlCoarse(_Handle):
    """Coarse frequency offset estimate (reference lib/pl_freq_sync.cc:93-199, lib/plsync_cc_impl.cc:567-606): per frame the
    autocorrelation of the modulation-removed PLHEADER (or SOF while not coarse-corrected and the PLSC is not known), summed
    over `period` frames; on a window's last frame the estimate and the coarse-corrected flag. The handle keeps the window's
    state on the device between calls. Outputs per frame: coarse_foffset float32, coarse_corrected int32, new_est int32."""
    _destroy = lib.dvbs2_plcoarse_destroy

    def __init__(self, period=1, plsc=-1, max_frames=1024, device=0):
        """plsc = -1: the PLSC comes with every frame (SOF form until coarse-corrected); 0..127: known, always the full form."""
        check(lib.dvbs2_plcoarse_create(C.byref(self._h), int(period), int(plsc), int(max_frames), device))
        self.period, self.plsc, self.max_frames = period, plsc, max_frames

    def reset(self):
        check(lib.dvbs2_plcoarse_reset(self._h))

    def work(self, plframes, plsc=None):
        """HOST buffer: complex64 [n_frames, stride] with stride >= 90 (only the first 90 symbols of a row are read); plsc: one
        integer per frame, or None for the handle's fixed PLSC. Returns dict(coarse_foffset, coarse_corrected, new_est)."""
        x = np.asarray(plframes)
        if x.dtype != np.complex64:
            raise TypeError(f"plframes must be complex64, not {x.dtype}")
        if x.ndim != 2 or x.shape[1] < 90 or not x.flags.c_contiguous:
            raise ValueError(f"plframes: a C-contiguous [n_frames, >= 90] array, got shape {x.shape}")
        nf = x.shape[0]
        if nf > self.max_frames:
            raise ValueError(f"{nf} frames exceed max_frames = {self.max_frames}")
        p = None
        if plsc is not None:
            p = np.asarray(plsc)
            if p.shape != (nf,) or p.dtype.kind not in "iu" or (p.size and (p.min() < 0 or p.max() > 127)):
                raise ValueError(f"plsc: {nf} integers in 0..127")
            p = np.ascontiguousarray(p, np.uint8)
        elif self.plsc < 0:
            raise ValueError("a PlCoarse without a fixed PLSC needs plsc per frame")
        fo, cc, ne = np.zeros(nf, np.float32), np.zeros(nf, np.int32), np.zeros(nf, np.int32)
        check(lib.dvbs2_plcoarse_estimate(self._h, _ptr(x), int(x.shape[1]), p.ctypes.data if p is not None and nf else None,
                                          nf, fo.ctypes.data, cc.ctypes.data, ne.ctypes.data))
        return dict(coarse_foffset=fo, coarse_corrected=cc, new_est=ne)

    def work_device(self, d_plframes, stride_syms, n_frames, d_plsc=0, d_coarse_foffset=0, d_coarse_corrected=0, d_new_est=0, stream=0):
        """DEVICE addresses, asynchronous on `stream`: frame f starts at symbol f * stride_syms; d_plsc = 0: the fixed PLSC."""
        check(lib.dvbs2_plcoarse_estimate_device(self._h, d_plframes, int(stride_syms), d_plsc or None, int(n_frames), d_coarse_foffset or None,
                                                 d_coarse_corrected or None, d_new_est or None, stream or None))

    def work_records_device(self, d_syms, n_syms, base_index, d_frames, n_frames, d_coarse_foffset=0, d_coarse_corrected=0, d_new_est=0,
                            stream=0):
        """DEVICE addresses: a raw symbol buffer whose first symbol has absolute index base_index, and the first n_frames records
        PlSync.work_device left for it."""
        check(lib.dvbs2_plcoarse_estimate_records_device(self._h, d_syms, int(n_syms), int(base_index), d_frames, int(n_frames),
                                                         d_coarse_foffset or None, d_coarse_corrected or None, d_new_est or None, stream or None))


def plsync_batch_check(plsc=-1, unlock_thresh=3, max_streams=1, max_symbols=1 << 20, max_frames=1024):
    """Raises Dvbs2Error (EINVAL, the text names the argument) for arguments a PlSyncBatch refuses. Host only."""
    check(lib.dvbs2_plsync_batch_check(int(plsc), int(unlock_thresh), int(max_streams), int(max_symbols), int(max_frames)))


def _stream_ints(v, n_streams, name):
    a = np.ascontiguousarray(v, np.int32).reshape(-1)
    if a.size != n_streams:
        raise ValueError(f"{name}: one integer per stream ({n_streams}), got {a.size}")
    return a


class PlSyncBatch(_Handle):
    """PlSync for a batch of independent symbol streams in one handle: one tracker, with its own state and history, per stream, and
    the launches of one search for any number of streams. Stream s of a batch gives the bits a PlSync of its own gives. The gather
    step writes SLOTS of plframe_len + 90 symbols -- a frame and the header that follows it in its own stream -- which
    PlCoarseBatch and PlFrontEnd.work_strided_device read; slots of all streams share one launch of each."""
    _destroy = lib.dvbs2_plsync_batch_destroy

    FRAME_DTYPE = PlSync.FRAME_DTYPE
    MIN_SYMBOLS = PlSync.MIN_SYMBOLS
    MAX_STREAMS = 1024

    def __init__(self, plsc=-1, unlock_thresh=3, max_streams=1, max_symbols=1 << 20, max_frames=1024, device=0, coherent=True, soft=True,
                 expected_pls=None):
        """max_symbols and max_frames are per stream. plsc = -1: decode the PLSC of every header; 0..127: the fixed-PLSC mode."""
        check(lib.dvbs2_plsync_batch_create(C.byref(self._h), int(plsc), int(unlock_thresh), int(max_streams), int(max_symbols), int(max_frames),
                                            device))
        self.plsc, self.unlock_thresh, self.max_streams, self.max_symbols, self.max_frames = plsc, unlock_thresh, max_streams, max_symbols, max_frames
        self.set_plsc_mode(coherent, soft)
        if expected_pls is not None:
            self.set_expected_pls(expected_pls)

    def reset(self):
        check(lib.dvbs2_plsync_batch_reset(self._h))

    def reset_stream(self, stream_index):
        check(lib.dvbs2_plsync_batch_reset_stream(self._h, int(stream_index)))

    def set_plsc_mode(self, coherent=True, soft=True):
        check(lib.dvbs2_plsync_batch_set_plsc_mode(self._h, int(bool(coherent)), int(bool(soft))))

    def set_expected_pls(self, plsc_list):
        """The enabled-codeword list, in the given order (empty: all 128)."""
        lst = np.asarray(plsc_list)
        if lst.size and (lst.dtype.kind not in "iu" or lst.min() < 0 or lst.max() > 127):
            raise ValueError("expected_pls: integers in 0..127")
        lst = np.ascontiguousarray(lst, np.uint8)
        check(lib.dvbs2_plsync_batch_set_expected_pls(self._h, _ptr(lst), int(lst.size)))

    def work_device(self, d_syms, stride_syms, first, n_syms, d_frames, stream=0):
        """DEVICE addresses, asynchronous on `stream`. first, n_syms: one integer per stream (host); stream s reads n_syms[s] symbols
        from symbol s * stride_syms + first[s] of d_syms. d_frames: [n_streams, max_frames] records of FRAME_DTYPE."""
        n = _stream_ints(n_syms, np.size(n_syms), "n_syms")
        f = _stream_ints(first, n.size, "first")
        self._n_streams = int(n.size)
        check(lib.dvbs2_plsync_batch_search_device(self._h, d_syms, int(stride_syms), f.ctypes.data, n.ctypes.data, int(n.size), d_frames, stream or None))

    def finish(self):
        """Waits for the last work_device(); returns (n_frames, consumed, state), each an int32 array over its streams."""
        v = [np.zeros(getattr(self, "_n_streams", 0), np.int32) for _ in range(3)]
        check(lib.dvbs2_plsync_batch_finish(self._h, *[a.ctypes.data for a in v]))
        return tuple(v)

    def gather_device(self, d_syms, stride_syms, d_frames, n_streams, wanted_plsc, d_slots, max_slots, d_offsets, d_slot_record=0, stream=0):
        """DEVICE addresses: the locked frames of wanted_plsc of the LAST work_device(), each with the 90 symbols behind it, into
        slots of plframe_len + 90 symbols, stream-major; d_offsets: n_streams + 1 int32 prefix sums of the true counts; slots at or
        beyond max_slots are not written; d_slot_record: per slot (stream, record index) as two int32, or 0."""
        check(lib.dvbs2_plsync_batch_gather_device(self._h, d_syms, int(stride_syms), d_frames, int(n_streams), int(wanted_plsc), d_slots or None,
                                                   int(max_slots), d_offsets, d_slot_record or None, stream or None))


class PlCoarseBatch(_Handle):
    """PlCoarse over the slots of PlSyncBatch.gather_device: one window state per stream, the slot ranges read from d_offsets on the
    device. Outputs per slot, the arrays PlFrontEnd.work_strided_device reads; stream s's are the bits a PlCoarse of its own gives."""
    _destroy = lib.dvbs2_plcoarse_batch_destroy

    def __init__(self, period=1, plsc=-1, max_streams=1, max_slots=1024, device=0):
        check(lib.dvbs2_plcoarse_batch_create(C.byref(self._h), int(period), int(plsc), int(max_streams), int(max_slots), device))
        self.period, self.plsc, self.max_streams, self.max_slots = period, plsc, max_streams, max_slots

    def reset(self):
        check(lib.dvbs2_plcoarse_batch_reset(self._h))

    def reset_stream(self, stream_index):
        check(lib.dvbs2_plcoarse_batch_reset_stream(self._h, int(stream_index)))

    def work_device(self, d_slots, stride_syms, d_offsets, n_streams, d_plsc=0, d_coarse_foffset=0, d_coarse_corrected=0, d_new_est=0, stream=0):
        """DEVICE addresses, asynchronous on `stream`: slot i starts at symbol i * stride_syms; d_plsc = 0: the fixed PLSC."""
        check(lib.dvbs2_plcoarse_batch_estimate_device(self._h, d_slots, int(stride_syms), d_plsc or None, d_offsets, int(n_streams),
                                                       d_coarse_foffset or None, d_coarse_corrected or None, d_new_est or None, stream or None))


def agc_check(rate, reference, gain, max_gain):
    """Raises Dvbs2Error (EINVAL, the text names the argument) for parameters an Agc refuses: a value that is not finite, a negative
    rate, a negative max_gain. max_gain == 0 means no cap. Host only."""
    check(lib.dvbs2_agc_check(float(rate), float(reference), float(gain), float(max_gain)))


class Agc(_Handle):
    """Automatic gain control, the stage in front of Rotator: GNU Radio's analog.agc_cc with max_gain behind an optional swap_iq
    (reference apps/dvbs2-rx:873-887), on a batch of independent streams whose gains stay on the device between calls
    (notes/agc.md). Per sample: y = x g; g += rate (reference - |y|); g capped at max_gain when max_gain > 0. All in float32."""
    _destroy = lib.dvbs2_agc_destroy

    TILE = capi.AGC_TILE

    def __init__(self, rate=1e-5, reference=1.0, gain=1.0, max_gain=65536.0, max_streams=1, max_samples=1 << 20, device=0):
        check(lib.dvbs2_agc_create(C.byref(self._h), float(rate), float(reference), float(gain), float(max_gain), int(max_streams),
                                   int(max_samples), device))
        self.max_streams, self.max_samples = max_streams, max_samples

    def params(self):
        """dict(rate, reference, max_gain as float32, swap_iq, tile)."""
        f, v = [C.c_float() for _ in range(3)], [C.c_int() for _ in range(2)]
        check(lib.dvbs2_agc_params(self._h, *[C.byref(x) for x in f], *[C.byref(x) for x in v]))
        return dict(rate=np.float32(f[0].value), reference=np.float32(f[1].value), max_gain=np.float32(f[2].value), swap_iq=bool(v[0].value),
                    tile=v[1].value)

    def reset(self):
        """Every stream's gain back to the gain of the constructor; waits for the device."""
        check(lib.dvbs2_agc_reset(self._h))

    def set_params(self, rate, reference, max_gain):
        """For the calls made after it."""
        check(lib.dvbs2_agc_set_params(self._h, float(rate), float(reference), float(max_gain)))

    def set_swap_iq(self, enable):
        check(lib.dvbs2_agc_set_swap_iq(self._h, int(bool(enable))))

    def set_gain(self, stream_index, gain):
        """One stream's gain (stream_index -1: every stream's); waits for the device."""
        check(lib.dvbs2_agc_set_gain(self._h, int(stream_index), float(gain)))

    def state(self, n_streams=None):
        """The gains of streams 0 .. n_streams - 1 (default: all) as float32; waits for the device."""
        g = np.zeros(self.max_streams if n_streams is None else int(n_streams), np.float32)
        check(lib.dvbs2_agc_state(self._h, _ptr(g), int(g.size)))
        return g

    def work(self, samples):
        """HOST buffer of complex64 samples of stream 0. Returns (out complex64, gain float32: what multiplied each sample)."""
        x = _complex64(samples, "samples")
        out, gain = np.empty_like(x), np.empty(x.size, np.float32)
        check(lib.dvbs2_agc_work(self._h, _ptr(x), int(x.size), _ptr(out), _ptr(gain)))
        return out, gain

    def work_device(self, d_in, in_stride, n_samples, n_streams, d_out, out_stride, d_gain=0, gain_stride=0, stream=0):
        """DEVICE addresses (samples 8-byte aligned), asynchronous on `stream`: stream s reads n_samples complex64 samples at
        d_in + 8 * s * in_stride, writes as many at d_out + 8 * s * out_stride and, when d_gain is given, n_samples float32 gains at
        d_gain + 4 * s * gain_stride. d_out == d_in with equal strides works in place. One call in flight per handle."""
        check(lib.dvbs2_agc_work_device(self._h, d_in or None, int(in_stride), int(n_samples), int(n_streams), d_out or None, int(out_stride),
                                        d_gain or None, int(gain_stride), stream or None))


_U64 = (1 << 64) - 1


def awgn_sigma(esn0_db, es=1.0, sps=1):
    """Per-component standard deviation (float32) of the noise that gives Es/N0 = esn0_db for symbol energy es at sps samples per symbol:
    N0 = es / 10^(esn0_db/10), sigma = sqrt(N0 sps / 2) (reference apps/dvbs2-tx:574-580), in double, rounded once. Host only."""
    s = C.c_float()
    check(lib.dvbs2_awgn_sigma(float(esn0_db), float(es), int(sps), C.byref(s)))
    return np.float32(s.value)


def awgn_words(seed, stream_id, index):
    """(wa, wb): the two Philox4x32-10 words behind complex sample `index` of stream `stream_id` under `seed`. Host only."""
    w = np.zeros(2, np.uint32)
    check(lib.dvbs2_awgn_words(int(seed) & _U64, int(stream_id) & _U64, int(index), w.ctypes.data))
    return int(w[0]), int(w[1])


def awgn_sample(seed, stream_id, index):
    """The unit-variance noise (re, im as float32) of complex sample `index` of stream `stream_id` under `seed`: the host compilation
    of the device's arithmetic, the same bits. Host only."""
    v = np.zeros(2, np.float32)
    check(lib.dvbs2_awgn_sample(int(seed) & _U64, int(stream_id) & _U64, int(index), v.ctypes.data))
    return v


def awgn_check(sigma, max_streams=1, max_samples=1):
    """Raises Dvbs2Error (EINVAL, the text names the argument) for what an Awgn refuses: a sigma that is negative or not finite,
    max_streams outside 1..65535, max_samples outside 1..2^30. Host only."""
    check(lib.dvbs2_awgn_check(float(sigma), int(max_streams), int(max_samples)))


class Awgn(_Handle):
    """Additive white Gaussian noise channel, the stage behind PulseShaper and in front of Rotator (reference apps/dvbs2-tx:572-584):
    y = x + sigma * noise per component, the noise a pure function of (seed, stream id, absolute sample index) -- Philox4x32-10 words
    through a float32 Box-Muller (notes/awgn.md). No device state: any number of calls may be in flight, and pieces equal one call.
    `position` is a host convenience: the first_index of a call that names none, advanced by n_samples by every such call."""
    _destroy = lib.dvbs2_awgn_destroy

    TILE = capi.AWGN_TILE

    def __init__(self, seed=0, sigma=0.0, max_streams=1, max_samples=1 << 20, device=0):
        check(lib.dvbs2_awgn_create(C.byref(self._h), int(seed) & _U64, float(sigma), int(max_streams), int(max_samples), device))
        self.max_streams, self.max_samples = max_streams, max_samples
        self.position = 0

    def params(self):
        """dict(seed, sigma as float32, max_streams, max_samples)."""
        seed, sigma, v = C.c_uint64(), C.c_float(), [C.c_int() for _ in range(2)]
        check(lib.dvbs2_awgn_params(self._h, C.byref(seed), C.byref(sigma), *[C.byref(x) for x in v]))
        return dict(seed=seed.value, sigma=np.float32(sigma.value), max_streams=v[0].value, max_samples=v[1].value)

    def set_sigma(self, sigma):
        """For the calls made after it."""
        check(lib.dvbs2_awgn_set_sigma(self._h, float(sigma)))

    def set_seed(self, seed):
        """For the calls made after it."""
        check(lib.dvbs2_awgn_set_seed(self._h, int(seed) & _U64))

    def work(self, samples, stream_id=0, first_index=None):
        """HOST buffer of complex64 samples of one stream, or an int: that many samples of the noise alone. Returns complex64."""
        if isinstance(samples, (int, np.integer)):
            x, n = None, int(samples)
        else:
            x = _complex64(samples, "samples")
            n = x.size
        out = np.empty(max(n, 0), np.complex64)
        first = self.position if first_index is None else int(first_index)
        check(lib.dvbs2_awgn_add(self._h, _ptr(x), n, int(stream_id) & _U64, first, _ptr(out)))
        if first_index is None:
            self.position += n
        return out

    def work_device(self, d_in, in_stride, n_samples, n_streams, d_out, out_stride, first_stream=0, first_index=None, d_sigma=0, stream=0):
        """DEVICE addresses (samples 8-byte aligned), asynchronous on `stream`: row r is stream first_stream + r, reads n_samples
        complex64 samples at d_in + 8 * r * in_stride (d_in 0: the noise alone) and writes as many at d_out + 8 * r * out_stride; its
        sample i has the absolute index first_index + i. d_sigma: n_streams float32, one per row, in place of the handle's sigma.
        d_out == d_in with equal strides works in place."""
        first = self.position if first_index is None else int(first_index)
        check(lib.dvbs2_awgn_add_device(self._h, d_in or None, int(in_stride), int(n_samples), int(n_streams), int(first_stream) & _U64, first,
                                        d_sigma or None, d_out or None, int(out_stride), stream or None))
        if first_index is None:
            self.position += int(n_samples)


IQ_FORMATS = {"u8": capi.IQ_U8, "s8": capi.IQ_S8, "s16": capi.IQ_S16}
_IQ_DTYPES = {capi.IQ_U8: np.uint8, capi.IQ_S8: np.int8, capi.IQ_S16: np.int16}


def _iq_format(fmt):
    return IQ_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


def _iq_codes(fmt, codes):
    """codes as a C-contiguous array of the format's dtype with an even number of elements (I, Q, I, Q, ...); any shape."""
    c = np.asarray(codes)
    if c.dtype != _IQ_DTYPES[fmt]:
        raise TypeError(f"codes must be {np.dtype(_IQ_DTYPES[fmt])}, not {c.dtype}")
    if not c.flags.c_contiguous or c.size % 2:
        raise ValueError("codes must be C-contiguous and hold whole samples (I, Q)")
    return c


def _iq_stats(words):
    return dict(samples=int(words[0]), clipped=int(words[1]), energy=int(words[2]))


def iqconv_bytes(fmt):
    """Bytes per complex sample of a format ("u8", "s8", "s16" or its number); -1 for an unknown number. Host only."""
    return lib.dvbs2_iqconv_bytes(_iq_format(fmt))


def iqconv_check(fmt, gain=1.0, max_streams=1, max_samples=1):
    """Raises Dvbs2Error (EINVAL, the text names the argument) for what an IqConverter refuses: an unknown format, a gain that is not
    finite, not positive or outside [2^-64, 2^64], max_streams outside 1..65535, max_samples outside 1..2^30. Host only."""
    check(lib.dvbs2_iqconv_check(_iq_format(fmt), float(gain), int(max_streams), int(max_samples)))


def iqconv_unpack_host(fmt, gain, codes, stats=False):
    """The host compilation of the device's arithmetic: codes (I, Q, I, Q, ... of the format's dtype) to complex64. With stats, also
    dict(samples, clipped, energy). Host only."""
    f = _iq_format(fmt)
    c = _iq_codes(f, codes)
    out = np.empty(c.size // 2, np.complex64)
    words = np.zeros(3, np.uint64)
    check(lib.dvbs2_iqconv_unpack_host(f, float(gain), _ptr(c), c.size // 2, _ptr(out), words.ctypes.data if stats else None))
    return (out, _iq_stats(words)) if stats else out


def iqconv_pack_host(fmt, gain, samples, stats=False):
    """The host compilation of the device's arithmetic: complex64 samples to codes [n, 2] of the format's dtype. With stats, also
    dict(samples, clipped, energy). Host only."""
    f = _iq_format(fmt)
    x = np.ascontiguousarray(samples, np.complex64).reshape(-1)
    out = np.empty((x.size, 2), _IQ_DTYPES[f])
    words = np.zeros(3, np.uint64)
    check(lib.dvbs2_iqconv_pack_host(f, float(gain), _ptr(x), x.size, _ptr(out), words.ctypes.data if stats else None))
    return (out, _iq_stats(words)) if stats else out


class IqConverter(_Handle):
    """IQ sample converter, the stage at the ends of both flowgraphs (reference apps/dvbs2-rx:685-707, apps/dvbs2-tx:533-549): interleaved
    u8 / s8 / s16 codes to complex64 samples (unpack, y = (c - B) / F * gain) and back (pack, rint(x * gain * F + B) clamped), with exact
    integer statistics {samples, clipped, energy} added per row to a caller's buffer (notes/iqconv.md). No device state: any number of
    device calls may be in flight."""
    _destroy = lib.dvbs2_iqconv_destroy

    TILE = capi.IQCONV_TILE

    def __init__(self, fmt="u8", gain=1.0, max_streams=1, max_samples=1 << 20, device=0):
        self.format = _iq_format(fmt)
        check(lib.dvbs2_iqconv_create(C.byref(self._h), self.format, float(gain), int(max_streams), int(max_samples), device))
        self.dtype = np.dtype(_IQ_DTYPES[self.format])
        self.bytes = lib.dvbs2_iqconv_bytes(self.format)
        self.max_streams, self.max_samples = max_streams, max_samples

    def params(self):
        """dict(format, gain as float32, max_streams, max_samples, tile)."""
        gain, v = C.c_float(), [C.c_int() for _ in range(4)]
        check(lib.dvbs2_iqconv_params(self._h, C.byref(v[0]), C.byref(gain), *[C.byref(x) for x in v[1:]]))
        return dict(format=v[0].value, gain=np.float32(gain.value), max_streams=v[1].value, max_samples=v[2].value, tile=v[3].value)

    def set_gain(self, gain):
        """For the calls made after it."""
        check(lib.dvbs2_iqconv_set_gain(self._h, float(gain)))

    def unpack_device(self, d_in, in_stride, n_samples, n_streams, d_out, out_stride, d_stats=0, stream=0):
        """DEVICE addresses, asynchronous on `stream`: row r reads n_samples samples of codes at d_in + bytes * r * in_stride (any byte
        address; s16: any even one) and writes as many complex64 at d_out + 8 * r * out_stride (8-byte aligned). d_stats: n_streams x 3
        uint64, added to."""
        check(lib.dvbs2_iqconv_unpack_device(self._h, d_in or None, int(in_stride), int(n_samples), int(n_streams), d_out or None, int(out_stride),
                                             d_stats or None, stream or None))

    def pack_device(self, d_in, in_stride, n_samples, n_streams, d_out, out_stride, d_stats=0, stream=0):
        """DEVICE addresses, asynchronous on `stream`: row r reads n_samples complex64 at d_in + 8 * r * in_stride and writes as many
        samples of codes at d_out + bytes * r * out_stride. d_stats: n_streams x 3 uint64, added to."""
        check(lib.dvbs2_iqconv_pack_device(self._h, d_in or None, int(in_stride), int(n_samples), int(n_streams), d_out or None, int(out_stride),
                                           d_stats or None, stream or None))

    def unpack_to_device(self, codes, d_out, stats=False):
        """HOST codes (I, Q, I, Q, ... of the format's dtype) to complex64 at the DEVICE address d_out; synchronous, only the codes cross
        the host link. With stats, returns dict(samples, clipped, energy)."""
        c = _iq_codes(self.format, codes)
        words = np.zeros(3, np.uint64)
        check(lib.dvbs2_iqconv_unpack_to_device(self._h, _ptr(c), c.size // 2, d_out or None,
                                                words.ctypes.data if stats else None))
        return _iq_stats(words) if stats else None

    def pack_from_device(self, d_in, n_samples, stats=False):
        """n_samples complex64 at the DEVICE address d_in to HOST codes [n_samples, 2]; synchronous. With stats, also the dict."""
        out = np.empty((max(int(n_samples), 0), 2), self.dtype)
        words = np.zeros(3, np.uint64)
        check(lib.dvbs2_iqconv_pack_from_device(self._h, d_in or None, int(n_samples), _ptr(out),
                                                words.ctypes.data if stats else None))
        return (out, _iq_stats(words)) if stats else out


class Rotator(_Handle):
    """Frequency-correcting rotator (reference lib/rotator_cc_impl.cc:36-128): out[n] = in[n] exp(j phi[n]), phi advancing by the
    phase increment per sample; increments change at once (set_phase_inc) or at scheduled absolute sample indices (schedule).
    Evaluated in closed form from a 64-bit fixed-point phase, not by the reference's phasor recurrence."""
    _destroy = lib.dvbs2_rotator_destroy

    def __init__(self, phase_inc=0.0, device=0):
        check(lib.dvbs2_rotator_create(C.byref(self._h), float(phase_inc), device))

    def reset(self):
        check(lib.dvbs2_rotator_reset(self._h))

    def set_phase_inc(self, phase_inc):
        check(lib.dvbs2_rotator_set_phase_inc(self._h, float(phase_inc)))

    def schedule(self, offset, phase_inc):
        """Queue `phase_inc` for the absolute sample index `offset`."""
        check(lib.dvbs2_rotator_schedule(self._h, int(offset), float(phase_inc)))

    def seek(self, n_syms):
        """Advance counter and phase over n_syms samples as calls would, without data."""
        check(lib.dvbs2_rotator_seek(self._h, int(n_syms)))

    def position(self):
        """(sample counter, queued updates)."""
        n, q = C.c_int64(), C.c_int()
        check(lib.dvbs2_rotator_position(self._h, C.byref(n), C.byref(q)))
        return n.value, q.value

    def work(self, syms):
        """HOST buffer of complex64 symbols; returns the rotated copy."""
        x = _complex64(syms, "syms")
        out = np.empty_like(x)
        check(lib.dvbs2_rotator_rotate(self._h, _ptr(x), int(x.size), _ptr(out)))
        return out

    def work_device(self, d_in, n_syms, d_out, stream=0):
        """DEVICE addresses (8-byte aligned), asynchronous on `stream`; d_out == d_in rotates in place."""
        check(lib.dvbs2_rotator_rotate_device(self._h, d_in, int(n_syms), d_out, stream or None))


ROTATOR_STATE = np.dtype(capi.ROTATOR_STATE_DTYPE)  # dvbs2_rotator_state_t: phase and inc in 2^-64 turns, index, reserved


def rotator_state_init(phase_inc):
    """One ROTATOR_STATE record per increment (radians per sample): phase 0 at index 0, the increment converted as Rotator converts
    it, so that a row started this way equals Rotator(phase_inc[s]) bit for bit. Host only; copy the array to the device."""
    inc = np.ascontiguousarray(phase_inc, np.float64).reshape(-1)
    state = np.zeros(inc.size, ROTATOR_STATE)
    check(lib.dvbs2_rotator_state_init(_ptr(inc), int(inc.size), _ptr(state)))
    return state


def rotator_state_read(state):
    """(phase_inc, phase_at_index) of HOST records as radians in (-pi, pi], one float64 array each. For printing and tests."""
    st = np.ascontiguousarray(state, ROTATOR_STATE).reshape(-1)
    inc, phase = np.zeros(st.size), np.zeros(st.size)
    check(lib.dvbs2_rotator_state_read(_ptr(st), int(st.size), _ptr(inc), _ptr(phase)))
    return inc, phase


def rotator_adjust_turns(estimate, scale):
    """(delta, applies): the control step's one conversion of an estimate (float32) and a scale (float64) into the 2^-64 turns that
    rotator_control_device subtracts from an increment; applies is False for a product that is not finite or not below 0.5 turns.
    Host only."""
    delta, applies = C.c_int64(), C.c_int()
    check(lib.dvbs2_rotator_adjust_turns(float(np.float32(estimate)), float(scale), C.byref(delta), C.byref(applies)))
    return delta.value, bool(applies.value)


def rotator_rows_device(d_in, in_stride, d_out, out_stride, n_samples, n_streams, base_index, d_state, device=0, stream=0):
    """DEVICE addresses (samples 8-byte aligned, d_state n_streams ROTATOR_STATE records, 16-byte aligned), asynchronous on `stream`,
    one launch: row s reads n_samples complex64 samples at d_in + 8 * s * in_stride, rotates sample i by its record's phase at the
    absolute index base_index + i and writes it at d_out + 8 * s * out_stride. The records are only read. d_out == d_in with equal
    strides works in place."""
    check(lib.dvbs2_rotator_rows_device(d_in or None, int(in_stride), d_out or None, int(out_stride), int(n_samples), int(n_streams),
                                        int(base_index), d_state or None, int(device), stream or None))


def rotator_retune_device(d_state, stream_index, at_index, phase_inc, device=0, stream=0):
    """DEVICE records: rebases record stream_index at the absolute index at_index and gives it the increment phase_inc (radians per
    sample); the phase stays continuous. Asynchronous on `stream`. Rotator.schedule(at_index, phase_inc) with the state on the device."""
    check(lib.dvbs2_rotator_retune_device(d_state or None, int(stream_index), int(at_index), float(phase_inc), int(device), stream or None))


def rotator_control_device(d_offsets, n_streams, max_slots, d_coarse_foffset, d_coarse_corrected, d_new_est, d_fine_foffset, d_fine_valid,
                           coarse_scale, fine_scale, at_index, d_state, d_applied=0, d_delta=0, device=0, stream=0):
    """DEVICE addresses, asynchronous on `stream`, one launch, nothing read back: the frequency-control step over the slots of one
    pass. Per stream the last qualifying slot decides (coarse: new_est and not coarse_corrected; fine: coarse_corrected and
    fine_valid); its estimate times its scale (gain / sps) is subtracted from the record's increment, rebased at at_index.
    d_fine_foffset / d_fine_valid: both or neither. d_applied: int32 per stream (0, 1 coarse, 2 fine, -1 did not apply); d_delta: int64."""
    check(lib.dvbs2_rotator_control_device(d_offsets or None, int(n_streams), int(max_slots), d_coarse_foffset or None, d_coarse_corrected or None,
                                           d_new_est or None, d_fine_foffset or None, d_fine_valid or None, float(coarse_scale), float(fine_scale),
                                           int(at_index), d_state or None, d_applied or None, d_delta or None, int(device), stream or None))


def symsync_loop_constants(sps, loop_bw, damping, rolloff):
    """(Kp, K1, K2) of the timing loop (reference lib/symbol_sync_cc_impl.cc:156-199) as float32. Host only."""
    v = [C.c_float() for _ in range(3)]
    check(lib.dvbs2_symsync_loop_constants(int(sps), float(loop_bw), float(damping), float(rolloff), *[C.byref(x) for x in v]))
    return tuple(np.float32(x.value) for x in v)


def symsync_geometry(sps, rrc_delay, n_subfilt, interp_method):
    """(subfilt_len, subfilt_delay, history) (reference lib/symbol_sync_cc_impl.cc:68-80, :244-256). Host only."""
    return _ints(3, lib.dvbs2_symsync_geometry, int(sps), int(rrc_delay), int(n_subfilt), int(interp_method))


def symsync_taps(sps, rolloff, rrc_delay, n_subfilt):
    """The polyphase RRC bank as float32 [n_subfilt, subfilt_len], each subfilter flipped (reference
    lib/symbol_sync_cc_impl.cc:82-110); the prototype is this library's own closed-form design. Host only."""
    L = symsync_geometry(sps, rrc_delay, n_subfilt, 0)[0]
    bank = np.empty((n_subfilt, L), np.float32)
    check(lib.dvbs2_symsync_taps(int(sps), float(rolloff), int(rrc_delay), int(n_subfilt), bank.ctypes.data))
    return bank


class SymbolSync(_Handle):
    """Symbol timing recovery (reference lib/symbol_sync_cc_impl.cc): Gardner detector, PI loop, modulo-1 counter and one of four
    interpolators (0 polyphase RRC bank = the matched filter, 1 linear, 2 quadratic, 3 cubic), on samples at `sps` per symbol.
    A call takes a batch of independent streams; the handle keeps each stream's loop state and history on the device between
    calls. Present a stream again from `consumed`, as with GNU Radio's consume()."""
    _destroy = lib.dvbs2_symsync_destroy

    POLYPHASE, LINEAR, QUADRATIC, CUBIC = 0, 1, 2, 3

    def __init__(self, sps=2, loop_bw=0.01, damping=1.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp_method=0, max_streams=1,
                 max_samples=1 << 20, device=0, taps=None):
        """taps: a float32 [n_subfilt, subfilt_len] bank to use instead of the library's design (symsync_taps' layout)."""
        args = (int(sps), float(loop_bw), float(damping), float(rolloff), int(rrc_delay), int(n_subfilt), int(interp_method))
        if taps is None:
            check(lib.dvbs2_symsync_create(C.byref(self._h), *args, int(max_streams), int(max_samples), device))
        else:
            t = np.ascontiguousarray(taps, np.float32)
            if t.shape != (n_subfilt, 2 * sps * rrc_delay + 1):
                raise ValueError(f"taps: [n_subfilt, subfilt_len] = {(n_subfilt, 2 * sps * rrc_delay + 1)}, got {t.shape}")
            check(lib.dvbs2_symsync_create_taps(C.byref(self._h), *args, t.ctypes.data, int(max_streams), int(max_samples), device))
        self.sps, self.interp_method, self.max_streams, self.max_samples = sps, interp_method, max_streams, max_samples
        v, f = [C.c_int() for _ in range(3)], [C.c_float() for _ in range(3)]
        check(lib.dvbs2_symsync_params(self._h, *[C.byref(x) for x in v], *[C.byref(x) for x in f]))
        self.subfilt_len, self.subfilt_delay, self.history = (x.value for x in v)
        self.Kp, self.K1, self.K2 = (np.float32(x.value) for x in f)
        self._n = 0

    def reset(self):
        check(lib.dvbs2_symsync_reset(self._h))

    def work_device(self, d_in, in_stride, n_in, d_out, out_stride, max_out, d_strobe_idx=0, d_mu=0, stream=0):
        """DEVICE addresses, asynchronous on `stream`; n_in: one sample count per stream (host). Stream s reads complex64 samples
        from d_in + 8 * s * in_stride and writes at most max_out symbols at d_out + 8 * s * out_stride (and int64 strobe indices /
        float64 mu at the same element stride). Read the result with finish()."""
        n = np.ascontiguousarray(np.atleast_1d(n_in), np.int32)
        self._n = n.size
        check(lib.dvbs2_symsync_work_device(self._h, d_in, int(in_stride), n.ctypes.data, int(n.size), d_out or None, int(out_stride), int(max_out),
                                            d_strobe_idx or None, d_mu or None, stream or None))

    def finish(self):
        """Waits for the last work_device(); returns (n_out, consumed, status), one int32 array each, per stream."""
        v = [np.zeros(max(self._n, 1), np.int32) for _ in range(3)]
        check(lib.dvbs2_symsync_finish(self._h, *[x.ctypes.data for x in v]))
        return tuple(x[:self._n] for x in v)

    def state(self, stream_index=0):
        """dict(vi, cnt, mu, n_read, last_xi, jump, init, status) of one stream; waits for the device."""
        s = capi.SymSyncState()
        check(lib.dvbs2_symsync_state(self._h, int(stream_index), C.byref(s)))
        return dict(vi=s.vi, cnt=s.cnt, mu=s.mu, n_read=s.n_read, last_xi=np.complex64(complex(s.last_xi_re, s.last_xi_im)), jump=s.jump,
                    init=s.init, status=s.status)

    def work(self, samples, max_out=None):
        """HOST buffer of complex64 samples of stream 0. Returns (symbols, strobe_idx int64, mu float64, consumed, status)."""
        x = _complex64(samples, "samples")
        if x.size > self.max_samples:
            raise ValueError(f"{x.size} samples exceed max_samples = {self.max_samples}")
        cap = x.size if max_out is None else int(max_out)
        out, idx, mu = np.zeros(cap, np.complex64), np.zeros(cap, np.int64), np.zeros(cap, np.float64)
        k, consumed, status = _ints(3, lib.dvbs2_symsync_work, self._h, _ptr(x), int(x.size),
                                    out.ctypes.data if cap else None, cap, idx.ctypes.data, mu.ctypes.data)
        return out[:k].copy(), idx[:k].copy(), mu[:k].copy(), consumed, status


def pl_scrambling_rn(gold_code, n):
    rn = np.zeros(n, np.uint8)
    check(lib.dvbs2_pl_scrambling_rn(gold_code, rn.ctypes.data, n))
    return rn


class BbDeheader(_Handle):
    """bbdeheader_bb (reference lib/bbdeheader_bb_impl.cc): descrambled BBFRAMEs in, 188-byte MPEG-TS packets out. The block's
    state (synchronised flag, partial packet, counters) is kept in the handle between calls, as between work() calls."""
    _destroy = lib.dvbs2_bbdeheader_destroy

    def __init__(self, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2", max_frames=64, device=0,
                 kbch_bits=None):
        if kbch_bits is not None:
            check(lib.dvbs2_bbdeheader_create_raw(C.byref(self._h), kbch_bits, max_frames, device))
        else:
            check(lib.dvbs2_bbdeheader_create(C.byref(self._h), standard, framesize, rate_id(rate), max_frames, device))
        self.kbch_bytes, self.max_dfl, self.max_out_bytes_per_frame = _ints(3, lib.dvbs2_bbdeheader_params, self._h)

    def work(self, bbframes):
        """bbframes: (n_frames, kbch_bytes) uint8 -> the TS bytes produced (general_work's output items)."""
        bb = np.ascontiguousarray(bbframes, dtype=np.uint8)
        nf = bb.shape[0] if bb.ndim == 2 else bb.size // self.kbch_bytes
        assert bb.size == nf * self.kbch_bytes
        out = np.empty(max(nf, 1) * self.max_out_bytes_per_frame, np.uint8)
        produced = C.c_int64()
        check(lib.dvbs2_bbdeheader_process(self._h, bb.ctypes.data, nf, out.ctypes.data, C.byref(produced)))
        return out[:produced.value].copy()

    def work_device(self, d_bbframes, n_frames, d_ts_out, stream=0):
        check(lib.dvbs2_bbdeheader_process_device(self._h, d_bbframes, n_frames, d_ts_out, stream))

    def finish(self, stream=0):
        produced = C.c_int64()
        check(lib.dvbs2_bbdeheader_finish(self._h, C.byref(produced), stream))
        return produced.value

    def counters(self, stream=0):
        c = capi.BbDeheaderCounters()
        check(lib.dvbs2_bbdeheader_counters(self._h, C.byref(c), stream))
        return {k: getattr(c, k) for k, _ in c._fields_}

    def reset(self, stream=0):
        check(lib.dvbs2_bbdeheader_reset(self._h, stream))


BBDEHEADER_STATE = np.dtype(capi.BBDEHEADER_STATE_DTYPE)  # dvbs2_bbdeheader_state_t, 256 bytes: all-zero bytes are the block as constructed


def bbdeheader_rows_check(kbch_bits, n_streams, max_frames):
    """None, or the text with which bbdeheader_rows_device refuses these ranges. Host only."""
    if lib.dvbs2_bbdeheader_rows_check(int(kbch_bits), int(n_streams), int(max_frames)) == capi.OK:
        return None
    return lib.dvbs2_last_error().decode()


def bbdeheader_rows_geometry(kbch_bits, n_streams, max_frames):
    """dict(kbch_bytes, max_out_bytes_per_frame, work_bytes, out_bytes): the sizes of a bbdeheader_rows_device call. Host only."""
    kb, mo, wb, ob = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
    check(lib.dvbs2_bbdeheader_rows_geometry(int(kbch_bits), int(n_streams), int(max_frames), C.byref(kb), C.byref(mo), C.byref(wb), C.byref(ob)))
    return dict(kbch_bytes=kb.value, max_out_bytes_per_frame=mo.value, work_bytes=wb.value, out_bytes=ob.value)


def bbdeheader_state_counters(state):
    """HOST records (BBDEHEADER_STATE) as one dict per stream with the keys of BbDeheader.counters()."""
    st = np.ascontiguousarray(state, BBDEHEADER_STATE).reshape(-1)
    out = (capi.BbDeheaderCounters * max(st.size, 1))()
    check(lib.dvbs2_bbdeheader_state_counters(_ptr(st), int(st.size), C.addressof(out)))
    return [{k: getattr(c, k) for k, _ in c._fields_} for c in out[:st.size]]


def bbdeheader_rows_device(d_bbframes, kbch_bits, d_offsets, n_streams, max_frames, d_state, d_work, work_bytes, d_ts_out, out_bytes,
                           d_pkt_offsets, device=0, stream=0):
    """DEVICE addresses, asynchronous on `stream`, five launches for any n_streams, nothing read back: stream s owns the BBFRAMEs
    d_offsets[s] .. d_offsets[s + 1] (int32, read on the device; those at or above max_frames are ignored) and its record d_state[s]
    (BBDEHEADER_STATE, 16-byte aligned). Its 188-byte packets go to d_ts_out at packet d_pkt_offsets[s], compact and stream-major;
    d_pkt_offsets gets n_streams + 1 int32. d_work / work_bytes and out_bytes: at least bbdeheader_rows_geometry's. The records are
    read and written: order calls on the same records or workspace on one stream."""
    check(lib.dvbs2_bbdeheader_rows_device(d_bbframes or None, int(kbch_bits), d_offsets or None, int(n_streams), int(max_frames), d_state or None,
                                           d_work or None, int(work_bytes), d_ts_out or None, int(out_bytes), d_pkt_offsets or None, int(device),
                                           stream or None))


def bbheader_build(matype1=0xF2, matype2=0, upl_bits=188 * 8, dfl_bits=0, sync=0x47, syncd_bits=0):
    """Ten BBHEADER bytes with their CRC-8 (host only)."""
    h = np.zeros(10, np.uint8)
    check(lib.dvbs2_bbheader_build(h.ctypes.data, matype1, matype2, upl_bits, dfl_bits, sync, syncd_bits))
    return h


def crc8(data):
    """The CRC-8 check byte of DVB-S2 mode adaptation over a bytes-like (host only)."""
    d = np.frombuffer(bytes(data), np.uint8)
    return check(lib.dvbs2_crc8(_ptr(d), d.size))


class BbFramer(_Handle):
    """BB framing, the mirror of BbDeheader: 188-byte MPEG-TS packets in, BBFRAMEs out (BBHEADER, a DATAFIELD of the CRC-encoded packet
    stream, zero padding). The position in the stream, the tail of a partly consumed packet and its CRC are kept in the handle between
    calls. dfl_bytes = 0: the largest DATAFIELD."""
    _destroy = lib.dvbs2_bbframer_destroy

    def __init__(self, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2", max_frames=64, device=0,
                 kbch_bits=None):
        if kbch_bits is not None:
            check(lib.dvbs2_bbframer_create_raw(C.byref(self._h), kbch_bits, max_frames, device))
        else:
            check(lib.dvbs2_bbframer_create(C.byref(self._h), standard, framesize, rate_id(rate), max_frames, device))
        self.kbch_bytes, self.max_dfl_bytes, self.max_packets_per_call = _ints(3, lib.dvbs2_bbframer_params, self._h)

    def set_matype(self, matype1=0xF2, matype2=0):
        check(lib.dvbs2_bbframer_set_matype(self._h, matype1, matype2))

    def need(self, n_frames, dfl_bytes=0):
        """Whole packets the next call (n_frames, dfl_bytes) reads (host only)."""
        return _ints(1, lib.dvbs2_bbframer_need, self._h, n_frames, dfl_bytes)[0]

    def work(self, ts, n_frames, dfl_bytes=0):
        """ts: at least need(n_frames, dfl_bytes) packets as uint8 -> (n_frames, kbch_bytes) uint8; self.packets_read says how many
        packets were taken."""
        t = np.ascontiguousarray(ts, dtype=np.uint8).reshape(-1)
        assert t.size >= 188 * self.need(n_frames, dfl_bytes)
        out = np.empty((max(n_frames, 0), self.kbch_bytes), np.uint8)
        n = C.c_int()
        check(lib.dvbs2_bbframer_process(self._h, _ptr(t), n_frames, dfl_bytes, _ptr(out), C.byref(n)))
        self.packets_read = n.value
        return out

    def work_device(self, d_ts, n_frames, d_bbframes, dfl_bytes=0, stream=0):
        check(lib.dvbs2_bbframer_process_device(self._h, d_ts, n_frames, dfl_bytes, d_bbframes, stream))

    def counters(self, stream=0):
        c = capi.BbFramerCounters()
        check(lib.dvbs2_bbframer_counters(self._h, C.byref(c), stream))
        return {k: getattr(c, k) for k, _ in c._fields_}

    def reset(self, stream=0):
        check(lib.dvbs2_bbframer_reset(self._h, stream))


class FecChain(_Handle):
    """demapper -> LDPC (OM_MESSAGE) -> BCH on the device, as wired in apps/dvbs2-rx:853-863. constellation: capi.MOD_QPSK,
    MOD_8PSK, MOD_16APSK or MOD_32APSK (the APSK chains run demapper -> LLR buffer -> LDPC, never the fused load)."""
    _destroy = lib.dvbs2_chain_destroy

    def __init__(self, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C3_4",
                 constellation=capi.MOD_8PSK, group_size=32, max_frames=64, max_trials=0, device=0, from_llr=False):
        if from_llr:  # ldpc_decoder_bb -> bch_decoder_bb only (LLRs in)
            check(lib.dvbs2_chain_create_llr(C.byref(self._h), standard, framesize, rate_id(rate), group_size, max_frames, device))
        else:
            check(lib.dvbs2_chain_create(C.byref(self._h), standard, framesize, rate_id(rate), constellation,
                                         group_size, max_frames, device))
        self._created(group_size, max_trials)

    @classmethod
    def from_table(cls, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C3_4", points=None, column=None, group_size=32,
                   max_frames=64, max_trials=0, device=0):
        """The chain with the demapper of a caller's table (Demapper.from_table: points, column); standard, framesize and rate
        choose the codes. Runs demapper -> LLR buffer -> LDPC -> BCH, never the fused load."""
        n_mod, pts, col = _table_args(points, column)
        self = cls.__new__(cls)
        check(lib.dvbs2_chain_create_table(C.byref(self._h), standard, framesize, rate_id(rate), n_mod, pts.ctypes.data,
                                           col.ctypes.data if col is not None else None, group_size, max_frames, device))
        self._created(group_size, max_trials)
        return self

    def _created(self, group_size, max_trials):
        a, b = C.c_int(), C.c_int()
        check(lib.dvbs2_chain_params(self._h, a, b))
        self.n_syms, self.msg_bytes = a.value, b.value
        check(lib.dvbs2_chain_llr_params(self._h, a, b, None))
        self.n_llr = a.value
        self.group_size = group_size
        self.max_trials = DEFAULT_TRIALS if max_trials == 0 else max_trials

    def set_descramble(self, enable=True):
        check(lib.dvbs2_chain_set_descramble(self._h, int(bool(enable))))

    def work(self, syms, n0, want_ret=True):
        """HOST buffers (dvbs2_chain_decode): syms complex64 [n_frames, n_syms] (or float32 [n_frames, 2 n_syms]), n0 scalar or
        one float per frame. Returns (msg uint8 [n_frames, msg_bytes], ldpc_ret int32 per group, bch_corr int32 per frame).
        Other complex / float widths are converted (the C entry reads float32 pairs); any other dtype is refused."""
        syms = np.asarray(syms)
        if syms.dtype.kind == "c":
            syms = np.ascontiguousarray(syms, np.complex64)
        elif syms.dtype.kind == "f":
            syms = np.ascontiguousarray(syms, np.float32)
        else:
            raise TypeError(f"symbols must be complex or float, not {syms.dtype}")
        n_frames = syms.shape[0]
        if syms.size * syms.itemsize != n_frames * self.n_syms * 8:
            raise ValueError(f"symbols: expected {n_frames} frames of {self.n_syms} complex values, got shape {syms.shape}")
        n0 = np.ascontiguousarray(np.atleast_1d(np.asarray(n0, np.float32)))
        msg = np.empty((n_frames, self.msg_bytes), np.uint8)
        ret = np.empty(((n_frames + self.group_size - 1) // self.group_size,), np.int32)
        corr = np.empty((n_frames,), np.int32)
        check(lib.dvbs2_chain_decode(self._h, syms.ctypes.data, n_frames, n0.ctypes.data, int(n0.size), self.max_trials,
                                     msg.ctypes.data, ret.ctypes.data if want_ret else None, corr.ctypes.data if want_ret else None))
        return msg, ret, corr

    def work_llr(self, llr, want_ret=True):
        """HOST buffers (dvbs2_chain_decode_llr): llr int8 [n_frames, N]."""
        llr = np.ascontiguousarray(llr, np.int8)
        n_frames = llr.shape[0]
        msg = np.empty((n_frames, self.msg_bytes), np.uint8)
        ret = np.empty(((n_frames + self.group_size - 1) // self.group_size,), np.int32)
        corr = np.empty((n_frames,), np.int32)
        check(lib.dvbs2_chain_decode_llr(self._h, llr.ctypes.data, n_frames, self.max_trials, msg.ctypes.data,
                                         ret.ctypes.data if want_ret else None, corr.ctypes.data if want_ret else None))
        return msg, ret, corr

    def work_host_ptr(self, syms_ptr, n_frames, n0_ptr, n0_count, msg_ptr, ret_ptr=0, corr_ptr=0):
        """dvbs2_chain_decode on raw HOST addresses (page-locked buffers of the caller: bench.py)."""
        check(lib.dvbs2_chain_decode(self._h, syms_ptr, n_frames, n0_ptr, n0_count, self.max_trials, msg_ptr, ret_ptr or None, corr_ptr or None))

    def work_device(self, d_syms, n_frames, d_n0, n0_count, d_msg, d_ldpc_ret=0, d_bch_corr=0, stream=0):
        check(lib.dvbs2_chain_decode_device(self._h, d_syms, n_frames, d_n0, n0_count, self.max_trials, d_msg,
                                            d_ldpc_ret or None, d_bch_corr or None, stream or None))

    def work_llr_device(self, d_llr, n_frames, d_msg, d_ldpc_ret=0, d_bch_corr=0, stream=0):
        check(lib.dvbs2_chain_decode_llr_device(self._h, d_llr, n_frames, self.max_trials, d_msg,
                                                d_ldpc_ret or None, d_bch_corr or None, stream or None))

    def enqueue_device(self, d_syms, n_frames, d_n0, n0_count, d_msg, d_ldpc_ret=0, d_bch_corr=0, stream=0):
        check(lib.dvbs2_chain_enqueue_device(self._h, d_syms, n_frames, d_n0, n0_count, self.max_trials, d_msg,
                                             d_ldpc_ret or None, d_bch_corr or None, stream or None))

    def enqueue_llr_device(self, d_llr, n_frames, d_msg, d_ldpc_ret=0, d_bch_corr=0, stream=0):
        check(lib.dvbs2_chain_enqueue_llr_device(self._h, d_llr, n_frames, self.max_trials, d_msg,
                                                 d_ldpc_ret or None, d_bch_corr or None, stream or None))

    def finish(self):
        check(lib.dvbs2_chain_finish(self._h))

    @property
    def kernel_name(self):
        return lib.dvbs2_chain_ldpc_kernel_name(self._h).decode()

    @property
    def fallback_rounds(self):
        """host-driven resolution rounds of the LDPC stage's group stop since creation (zero in normal operation)"""
        return lib.dvbs2_chain_ldpc_fallback_rounds(self._h)

    def profile(self, enable=True):
        ms, n = C.c_double(), C.c_int()
        check(lib.dvbs2_chain_ldpc_profile(self._h, 1 if enable else 0, ms, n))
        return ms.value, n.value


def enc_check(standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2", constellation=capi.ENC_NO_MAPPER):
    """Whether FecEncoder takes this MODCOD (dvbs2_enc_check; raises Dvbs2Error with the text that names the argument). Host only."""
    check(lib.dvbs2_enc_check(standard, framesize, rate_id(rate), constellation))


class FecEncoder(_Handle):
    """The forward direction of FecChain on the device: BBFRAME bytes -> [BB scrambler] -> BCH -> LDPC -> mapper, every result bit
    for bit (notes/encoder.md). constellation: capi.MOD_QPSK, MOD_8PSK, MOD_16APSK, MOD_32APSK or capi.ENC_NO_MAPPER. PL framing
    is not part of it (PlFramer takes the symbols on). The reference has no transmit blocks to mirror."""
    _destroy = lib.dvbs2_enc_destroy
    OUTPUTS = ("bch_cw", "ldpc_cw", "syms")

    def __init__(self, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2", constellation=capi.MOD_QPSK,
                 max_frames=64, device=0):
        check(lib.dvbs2_enc_create(C.byref(self._h), standard, framesize, rate_id(rate), constellation, max_frames, device))
        self._created()

    @classmethod
    def from_table(cls, standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_NORMAL, rate="C1_2", points=None, column=None,
                   max_frames=64, device=0):
        """The encoder with the mapper of a caller's table (points, column as for Demapper.from_table)."""
        n_mod, pts, col = _table_args(points, column)
        self = cls.__new__(cls)
        check(lib.dvbs2_enc_create_table(C.byref(self._h), standard, framesize, rate_id(rate), n_mod, pts.ctypes.data,
                                         col.ctypes.data if col is not None else None, max_frames, device))
        self._created()
        return self

    @classmethod
    def from_parts(cls, bch=None, ldpc_table=None, max_frames=64, device=0):
        """Single stages of any code the library knows: bch = (m, prim_poly, t, n) or None, ldpc_table = a table name or None.
        No mapper."""
        m, prim, t, n = bch if bch is not None else (0, 0, 0, 0)
        self = cls.__new__(cls)
        check(lib.dvbs2_enc_create_parts(C.byref(self._h), m, prim, t, n, ldpc_table.encode() if ldpc_table is not None else None,
                                         max_frames, device))
        self._created()
        return self

    def _created(self):
        self.in_bits, self.bch_n, self.ldpc_n, self.n_syms, self.n_mod = _ints(5, lib.dvbs2_enc_params, self._h)
        self.in_bytes = self.in_bits // 8

    def set_scramble(self, enable=True):
        """Fuse the BB scrambler (in ^= bb_descramble_sequence) into the BCH stage's load."""
        check(lib.dvbs2_enc_set_scramble(self._h, int(bool(enable))))

    def work(self, frames, want=None):
        """HOST buffers (dvbs2_enc_encode): frames uint8 [n_frames, in_bytes]. want: names out of OUTPUTS (default: every stage
        the encoder has). Returns a dict name -> array: bch_cw / ldpc_cw uint8 [n_frames, n / 8], syms complex64 [n_frames, n_syms]."""
        frames = np.ascontiguousarray(frames, np.uint8)
        nf = frames.shape[0]
        if frames.shape != (nf, self.in_bytes):
            raise ValueError(f"frames: expected (n_frames, {self.in_bytes}) bytes, got shape {frames.shape}")
        if want is None:
            want = [n for n, have in zip(self.OUTPUTS, (self.bch_n, self.ldpc_n, self.n_syms)) if have]
        out = {}
        for name in want:
            if name not in self.OUTPUTS:
                raise ValueError(f"unknown output {name}")
            out[name] = (np.empty((nf, self.n_syms), np.complex64) if name == "syms" else
                         np.empty((nf, (self.bch_n if name == "bch_cw" else self.ldpc_n) // 8), np.uint8))
        ptrs = [out[n].ctypes.data if n in out else None for n in self.OUTPUTS]
        check(lib.dvbs2_enc_encode(self._h, frames.ctypes.data, nf, *ptrs))
        return out

    def work_device(self, d_in, n_frames, d_bch_cw=0, d_ldpc_cw=0, d_syms=0, stream=0):
        check(lib.dvbs2_enc_encode_device(self._h, d_in, n_frames, d_bch_cw or None, d_ldpc_cw or None, d_syms or None, stream or None))


def _plsc_array(plscs):
    a = np.asarray(plscs)
    if a.ndim != 1 or (a.size and (a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 255)):
        raise ValueError("plscs: a vector of integers in 0..127")
    return np.ascontiguousarray(a, np.uint8)


def plframer_layout(plscs):
    """Where PlFramer reads and writes the frames of a sequence (dvbs2_plframer_layout): a dict of in_offset, out_offset (int64 per
    frame, in complex symbols; a dummy frame reads nothing) and the totals in_syms, out_syms. Host only."""
    a = _plsc_array(plscs)
    ino, outo = np.zeros(a.size, np.int64), np.zeros(a.size, np.int64)
    tin, tout = C.c_int64(), C.c_int64()
    check(lib.dvbs2_plframer_layout(_ptr(a), int(a.size), ino.ctypes.data, outo.ctypes.data, C.byref(tin), C.byref(tout)))
    return dict(in_offset=ino, out_offset=outo, in_syms=tin.value, out_syms=tout.value)


class PlFramer(_Handle):
    """PL framing, the step behind FecEncoder: PLHEADER, pilot blocks and PL scrambling of a sequence of frames with mixed MODCODs and
    dummy frames, every output bit for bit (notes/plframer.md). The input is the XFECFRAMEs of the non-dummy frames back to back."""
    _destroy = lib.dvbs2_plframer_destroy

    def __init__(self, gold_code=0, max_frames=16, device=0):
        check(lib.dvbs2_plframer_create(C.byref(self._h), int(gold_code), int(max_frames), device))
        self.gold_code, self.max_frames, self.plscs = gold_code, max_frames, np.zeros(0, np.uint8)
        self._params()

    def _params(self):
        n, tin, tout = C.c_int(), C.c_int64(), C.c_int64()
        check(lib.dvbs2_plframer_params(self._h, C.byref(n), C.byref(tin), C.byref(tout)))
        self.n_frames, self.in_syms, self.out_syms = n.value, tin.value, tout.value

    def set_sequence(self, plscs):
        """The PLSCs of the frames of one call, in stream order. Not while work of the handle is in flight."""
        a = _plsc_array(plscs)
        check(lib.dvbs2_plframer_set_sequence(self._h, _ptr(a), int(a.size)))
        self.plscs = a
        self._params()

    def work(self, xfecframes, n_frames=None, closing_plsc=-1):
        """HOST buffer: complex64, the XFECFRAMEs the first n_frames (default: all) of the sequence read, flat or any shape. Returns
        the PLFRAMEs back to back (+ the closing header) as a complex64 vector."""
        nf = self.n_frames if n_frames is None else int(n_frames)
        if not 0 <= nf <= self.n_frames:
            raise ValueError(f"n_frames: 0..{self.n_frames}")
        lay = plframer_layout(self.plscs[:nf])
        x = np.asarray(xfecframes)
        if x.dtype != np.complex64:
            raise TypeError(f"xfecframes must be complex64, not {x.dtype}")
        if not x.flags.c_contiguous or x.size != lay["in_syms"]:
            raise ValueError(f"xfecframes: expected {lay['in_syms']} C-contiguous symbols, got shape {x.shape}")
        out = np.empty(lay["out_syms"] + (90 if closing_plsc >= 0 and nf else 0), np.complex64)
        check(lib.dvbs2_plframer_frame(self._h, _ptr(x), nf, int(closing_plsc), _ptr(out)))
        return out

    def work_device(self, d_xfecframes, n_frames, closing_plsc, d_plframes, stream=0):
        """DEVICE addresses, asynchronous on `stream`: writes out_offset[n_frames] (+ 90 with a closing header) symbols."""
        check(lib.dvbs2_plframer_frame_device(self._h, d_xfecframes or None, int(n_frames), int(closing_plsc), d_plframes or None, stream or None))


def pulse_geometry(sps, rrc_delay):
    """(ntaps, history in symbols, delay in samples) of the pulse shaper's own design (dvbs2_pulse_geometry). Host only."""
    return _ints(3, lib.dvbs2_pulse_geometry, int(sps), int(rrc_delay))


def pulse_taps(sps, rolloff, rrc_delay, tau=0.0, gain=None):
    """The RRC taps of the pulse shaper as float32 [2 sps rrc_delay + 1]: the closed form behind symsync_taps, shifted by tau symbols
    (|tau| <= 0.5) and scaled so that the taps at tau = 0 sum to gain (default sps, firdes's convention). Host only."""
    taps = np.empty(pulse_geometry(sps, rrc_delay)[0], np.float32)
    check(lib.dvbs2_pulse_taps(int(sps), float(rolloff), int(rrc_delay), float(tau), float(sps if gain is None else gain), taps.ctypes.data))
    return taps


def pulse_scale_taps(taps, sps, fullscale=1.0):
    """A float32 copy of `taps` scaled by the rule of the reference's scale_rrc_taps (apps/dvbs2-tx:39-81): I and Q of the shaped
    samples of unit-magnitude symbols stay within +-fullscale. Host only."""
    t = np.array(taps, np.float32).reshape(-1)
    check(lib.dvbs2_pulse_scale_taps(_ptr(t), int(t.size), int(sps), float(fullscale)))
    return t


class PulseShaper(_Handle):
    """Pulse shaping, the step behind PlFramer: an interpolating FIR by the integer factor `sps` with real taps over complex symbols,
    on a batch of independent streams whose histories stay on the device between calls (notes/pulse_shaper.md). n symbols in give
    n * sps samples out, delayed by `delay` samples; flush with `history` zero symbols."""
    _destroy = lib.dvbs2_pulse_destroy

    TILE = capi.PULSE_TILE

    def __init__(self, sps=2, rolloff=0.2, rrc_delay=5, max_streams=1, max_symbols=1 << 20, device=0, taps=None):
        """taps: a float32 vector to use instead of the library's design (pulse_taps with tau = 0, gain = sps)."""
        if taps is None:
            check(lib.dvbs2_pulse_create(C.byref(self._h), int(sps), float(rolloff), int(rrc_delay), int(max_streams), int(max_symbols), device))
        else:
            t, t_ptr, ntaps = _f32_vector(taps)
            check(lib.dvbs2_pulse_create_taps(C.byref(self._h), int(sps), t_ptr, ntaps, int(max_streams), int(max_symbols), device))
        self.max_streams, self.max_symbols = max_streams, max_symbols
        self.sps, self.ntaps, self.history, self.delay = _ints(4, lib.dvbs2_pulse_params, self._h)

    def reset(self):
        check(lib.dvbs2_pulse_reset(self._h))

    def work(self, syms):
        """HOST buffer of complex64 symbols of stream 0; returns the syms.size * sps complex64 samples."""
        x = _complex64(syms, "syms")
        out = np.empty(x.size * self.sps, np.complex64)
        check(lib.dvbs2_pulse_shape(self._h, _ptr(x), int(x.size), _ptr(out)))
        return out

    def work_device(self, d_in, in_stride, n_syms, n_streams, d_out, out_stride, stream=0):
        """DEVICE addresses (8-byte aligned, not overlapping), asynchronous on `stream`: stream s reads n_syms complex64 symbols at
        d_in + 8 * s * in_stride and writes n_syms * sps samples at d_out + 8 * s * out_stride. One call in flight per handle."""
        check(lib.dvbs2_pulse_shape_device(self._h, d_in or None, int(in_stride), int(n_syms), int(n_streams), d_out or None, int(out_stride),
                                           stream or None))


def resamp_step(rate):
    """nearbyint(2^32 / rate) for rate in [0.5, 64]: input samples per output sample with 32 fractional bits (dvbs2_resamp_step). The
    effective rate is exactly 2^32 / step. Host only."""
    step = C.c_uint64()
    check(lib.dvbs2_resamp_step(float(rate), C.byref(step)))
    return step.value


def resamp_geometry(nfilts, ntaps):
    """(terms per branch L, history in samples, delay_num: the delay is delay_num / nfilts input samples) (dvbs2_resamp_geometry).
    Host only."""
    return _ints(3, lib.dvbs2_resamp_geometry, int(nfilts), int(ntaps))


def resamp_max_out(step, n_in):
    """The largest n_out of a call of n_in samples for any position (dvbs2_resamp_max_out). Host only."""
    n = lib.dvbs2_resamp_max_out(int(step), int(n_in))
    check(min(n, 0))
    return n


def resamp_check(nfilts, taps, rate, max_streams=1, max_samples=1 << 20):
    """Raises what Resampler(...) would raise for these arguments, without a device (dvbs2_resamp_check)."""
    t, t_ptr, ntaps = _f32_vector(taps)
    check(lib.dvbs2_resamp_check(int(nfilts), t_ptr, ntaps, float(rate), int(max_streams), int(max_samples)))


class Resampler(_Handle):
    """Arbitrary-rate resampling: a polyphase bank of `nfilts` branches of the caller's prototype `taps` with linear interpolation
    between neighbouring branches, real taps over complex samples, on a batch of independent streams whose histories and positions stay
    on the device between calls (notes/resampler.md). n samples in give about n * rate samples out -- produce(n) says exactly how many --
    delayed by delay_num / nfilts input samples; flush with `history` zero samples."""
    _destroy = lib.dvbs2_resamp_destroy

    TILE = capi.RESAMP_TILE

    def __init__(self, nfilts, taps, rate, max_streams=1, max_samples=1 << 20, device=0):
        t, t_ptr, ntaps = _f32_vector(taps)
        check(lib.dvbs2_resamp_create(C.byref(self._h), int(nfilts), t_ptr, ntaps, float(rate), int(max_streams), int(max_samples), device))
        self.max_streams, self.max_samples = max_streams, max_samples
        self.nfilts, self.ntaps, self.terms, self.history, self.delay_num = _ints(5, lambda *a: lib.dvbs2_resamp_params(*a, None), self._h)

    @property
    def step(self):
        step = C.c_uint64()
        check(lib.dvbs2_resamp_params(self._h, None, None, None, None, None, C.byref(step)))
        return step.value

    def set_rate(self, rate):
        """From the next call on; the positions are carried over."""
        check(lib.dvbs2_resamp_set_rate(self._h, float(rate)))

    def set_step(self, step):
        check(lib.dvbs2_resamp_set_step(self._h, int(step)))

    def reset(self):
        check(lib.dvbs2_resamp_reset(self._h))

    def reset_phase(self, frac=None):
        """Position of stream s = frac[s] / 2^32 input samples (max_streams values below 2^32; None: zeros). Histories stay."""
        if frac is None:
            check(lib.dvbs2_resamp_reset_phase(self._h, None))
            return
        f = np.ascontiguousarray(frac, np.uint32).reshape(-1)
        if f.size != self.max_streams:
            raise ValueError(f"frac: expected {self.max_streams} values, got {f.size}")
        check(lib.dvbs2_resamp_reset_phase(self._h, f.ctypes.data))

    def produce(self, n_in, n_streams=1):
        """int64 [n_streams]: what the next call of n_in samples writes per stream. From the host's mirror: no synchronisation."""
        n = np.zeros(int(n_streams), np.int64)
        check(lib.dvbs2_resamp_produce(self._h, int(n_in), int(n_streams), _ptr(n)))
        return n

    def state(self):
        """uint64 [max_streams]: the DEVICE's positions. Synchronous."""
        acc = np.zeros(self.max_streams, np.uint64)
        check(lib.dvbs2_resamp_state(self._h, acc.ctypes.data))
        return acc

    def work(self, samples):
        """HOST buffer of complex64 samples of stream 0; returns the produce(samples.size)[0] complex64 samples."""
        x = _complex64(samples, "samples")
        out = np.empty(max(int(self.produce(x.size)[0]), 1), np.complex64)
        n = C.c_int64()
        check(lib.dvbs2_resamp_process(self._h, _ptr(x), int(x.size), out.ctypes.data, int(out.size), C.byref(n)))
        return out[:n.value]

    def work_device(self, d_in, in_stride, n_in, n_streams, d_out, out_stride, stream=0):
        """DEVICE addresses (8-byte aligned, not overlapping), asynchronous on `stream`: stream s reads n_in complex64 samples at
        d_in + 8 * s * in_stride and writes n_out[s] samples at d_out + 8 * s * out_stride; out_stride >= max(n_out). Returns n_out as
        int64 [n_streams] (what produce() said before the call). One call in flight per handle."""
        n = np.zeros(int(n_streams), np.int64)
        check(lib.dvbs2_resamp_process_device(self._h, d_in or None, int(in_stride), int(n_in), int(n_streams), d_out or None, int(out_stride),
                                              _ptr(n), stream or None))
        return n


def ddc_geometry(decim, ntaps):
    """(history in mixed samples per channel, delay_num: the delay is delay_num / 2 input samples) (dvbs2_ddc_geometry). Host only."""
    return _ints(2, lib.dvbs2_ddc_geometry, int(decim), int(ntaps))


def ddc_produce(position, decim, n_in):
    """What a call of n_in samples writes per channel when the sample counter stands at `position`:
    ceil((position + n_in) / decim) - ceil(position / decim) (dvbs2_ddc_produce). Host only."""
    n = lib.dvbs2_ddc_produce(int(position), int(decim), int(n_in))
    check(min(n, 0))
    return n


def ddc_check(decim, taps, max_channels=1, max_inputs=1, max_samples=1 << 20):
    """Raises what Ddc(...) would raise for these arguments, without a device (dvbs2_ddc_check)."""
    t, t_ptr, ntaps = _f32_vector(taps)
    check(lib.dvbs2_ddc_check(int(decim), t_ptr, ntaps, int(max_channels), int(max_inputs), int(max_samples)))


def ddc_tile(decim, ntaps):
    """Output samples per workgroup of the down-converter's kernel: the tile rule of include/dvbs2_fec_hip.h. Host only."""
    return min(capi.DDC_MAX_TILE, (capi.DDC_SPAN - (int(ntaps) - 1)) // int(decim))


class Ddc(_Handle):
    """Digital down-conversion: a frequency-translating decimating FIR with the caller's real `taps`. Channel c reads input stream
    input[c], mixes it with its own phase increment (radians per input sample, the rotator's arithmetic), filters it and keeps every
    decim-th sample; the last ntaps - 1 mixed samples and the phase of every channel stay on the device between calls (notes/ddc.md).
    n samples in give produce(n) samples out per channel, delayed by delay_num / 2 input samples."""
    _destroy = lib.dvbs2_ddc_destroy

    def __init__(self, decim, taps, max_channels=1, max_inputs=1, max_samples=1 << 20, device=0):
        t, t_ptr, ntaps = _f32_vector(taps)
        check(lib.dvbs2_ddc_create(C.byref(self._h), int(decim), t_ptr, ntaps, int(max_channels), int(max_inputs), int(max_samples), device))
        self.max_channels, self.max_inputs, self.max_samples = max_channels, max_inputs, max_samples
        self.decim, self.ntaps, self.history, self.delay_num, self.tile = _ints(5, lib.dvbs2_ddc_params, self._h)

    def set_channel(self, channel, phase_inc, input=0):
        """From the next call on; the channel's phase is carried over."""
        check(lib.dvbs2_ddc_set_channel(self._h, int(channel), int(input), float(phase_inc)))

    def reset(self):
        check(lib.dvbs2_ddc_reset(self._h))

    def position(self):
        """The sample counter, from the host's mirror."""
        n = C.c_int64()
        check(lib.dvbs2_ddc_position(self._h, C.byref(n)))
        return n.value

    def channel(self, channel):
        """(input, increment, phase) of a channel from the host's mirror, the last two in 2^-64 turns."""
        i, inc, ph = C.c_int(), C.c_uint64(), C.c_uint64()
        check(lib.dvbs2_ddc_channel(self._h, int(channel), C.byref(i), C.byref(inc), C.byref(ph)))
        return i.value, inc.value, ph.value

    def produce(self, n_in):
        """What the next call of n_in samples writes per channel. From the host's mirror: no synchronisation."""
        return ddc_produce(self.position(), self.decim, n_in)

    def state(self):
        """uint64 [max_channels]: the DEVICE's phases in 2^-64 turns. Synchronous."""
        ph = np.zeros(self.max_channels, np.uint64)
        check(lib.dvbs2_ddc_state(self._h, ph.ctypes.data))
        return ph

    def work(self, samples, n_channels=None):
        """HOST buffer: complex64 [n_inputs, n_in] (or a vector: one input). Returns complex64 [n_channels, produce(n_in)]."""
        x = _complex64(samples, "samples", rows="[n_inputs, n_in]")
        nc = self.max_channels if n_channels is None else int(n_channels)
        n_inputs, n_in = x.shape
        stride = max(self.produce(n_in), 1) if n_in <= self.max_samples else 1
        out = np.empty((max(nc, 1), stride), np.complex64)
        n = C.c_int64()
        check(lib.dvbs2_ddc_process(self._h, _ptr(x), int(n_in), int(n_in), int(n_inputs), nc, out.ctypes.data,
                                    int(stride), C.byref(n)))
        return out[:nc, :n.value]

    def work_device(self, d_in, in_stride, n_in, n_inputs, n_channels, d_out, out_stride, stream=0):
        """DEVICE addresses (8-byte aligned, not overlapping), asynchronous on `stream`: channel c reads n_in complex64 samples at
        d_in + 8 * input[c] * in_stride and writes n_out samples at d_out + 8 * c * out_stride; out_stride >= n_out. Returns n_out (what
        produce() said before the call). One call in flight per handle."""
        n = C.c_int64()
        check(lib.dvbs2_ddc_process_device(self._h, d_in or None, int(in_stride), int(n_in), int(n_inputs), int(n_channels), d_out or None,
                                           int(out_stride), C.byref(n), stream or None))
        return n.value


SPECTRUM_WINDOWS = {"rect": capi.SPECTRUM_RECT, "hann": capi.SPECTRUM_HANN, "hamming": capi.SPECTRUM_HAMMING,
                    "blackman-harris": capi.SPECTRUM_BLACKMAN_HARRIS}


def spectrum_geometry(nfft, hop, avg, n_in):
    """(n_seg, n_rows, used_samples) of a call of n_in samples per stream (dvbs2_spectrum_geometry). Host only."""
    return _ints(3, lib.dvbs2_spectrum_geometry, int(nfft), int(hop), int(avg), int(n_in))


def spectrum_window(kind, nfft):
    """The periodic window `kind` ("rect", "hann", "hamming", "blackman-harris" or its number) as float32 [nfft]
    (dvbs2_spectrum_window). Host only."""
    w = np.zeros(max(int(nfft), 1), np.float32)
    check(lib.dvbs2_spectrum_window(SPECTRUM_WINDOWS.get(kind, kind), int(nfft), w.ctypes.data))
    return w


def spectrum_twiddles(nfft):
    """The transform's one table, complex64 [nfft / 2] (dvbs2_spectrum_twiddles). Host only."""
    t = np.zeros(max(int(nfft) // 2, 1), np.complex64)
    check(lib.dvbs2_spectrum_twiddles(int(nfft), t.ctypes.data))
    return t


def _window_arg(window, nfft):
    if window is None:
        return None
    if isinstance(window, (str, int)):
        return spectrum_window(window, nfft)
    w = _f32_vector(window)[0]
    if w.size != int(nfft):
        raise ValueError("the window must have nfft values")
    return w


def spectrum_check(nfft, hop, avg=0, window=None, max_streams=1, max_samples=1 << 20):
    """Raises what Spectrum(...) would raise for these arguments, without a device (dvbs2_spectrum_check)."""
    w = _window_arg(window, nfft)
    check(lib.dvbs2_spectrum_check(int(nfft), int(hop), int(avg), None if w is None else w.ctypes.data, int(max_streams), int(max_samples)))


def spectrum_carriers(psd, shifted=True, max_out=64, smooth=None, floor_quantile=None, threshold_db=None, min_gap=None, min_width=None):
    """The carriers of one row of a power spectrum (dvbs2_spectrum_carriers): a record array (capi.SPECTRUM_CARRIER_DTYPE) sorted by
    centre -- centre and bandwidth in cycles per sample, level and floor in the row's units, the edge bins -- and the number found,
    which may exceed max_out. Parameters left at None take the library's defaults. Host only."""
    row, row_ptr, nfft = _f32_vector(psd)
    params = None
    if any(v is not None for v in (smooth, floor_quantile, threshold_db, min_gap, min_width)):
        params = capi.SpectrumCarrierParams(0.25 if floor_quantile is None else float(floor_quantile), 6.0 if threshold_db is None else float(threshold_db),
                                            9 if smooth is None else int(smooth), 4 if min_gap is None else int(min_gap),
                                            8 if min_width is None else int(min_width), 0)
    out = np.zeros(max(int(max_out), 1), capi.SPECTRUM_CARRIER_DTYPE)
    n = C.c_int()
    check(lib.dvbs2_spectrum_carriers(row_ptr, nfft, int(bool(shifted)),
                                      C.addressof(params) if params is not None else None, out.ctypes.data, int(max_out), C.byref(n)))
    return out[:min(n.value, int(max_out))], n.value


class Spectrum(_Handle):
    """Power spectra of sample streams by Welch's method: segments of nfft samples every hop samples, windowed, transformed, their powers
    averaged over avg segments per row (avg = 0: all segments of a call in one row) and scaled so that white noise of variance sigma^2
    gives sigma^2 in every bin (notes/spectrum.md). No state between calls. window: None (periodic Hann), a name or number of
    spectrum_window, or nfft values. shifted: DC at index nfft / 2, else first."""
    _destroy = lib.dvbs2_spectrum_destroy

    def __init__(self, nfft, hop=None, avg=0, window=None, shifted=True, max_streams=1, max_samples=1 << 20, device=0):
        hop = int(nfft) // 2 if hop is None else hop
        w = _window_arg(window, nfft)
        check(lib.dvbs2_spectrum_create(C.byref(self._h), int(nfft), int(hop), int(avg), None if w is None else w.ctypes.data, int(bool(shifted)),
                                        int(max_streams), int(max_samples), device))
        self.max_streams, self.max_samples = max_streams, max_samples
        v, p = [C.c_int() for _ in range(4)], C.c_double()
        check(lib.dvbs2_spectrum_params(self._h, *v, C.byref(p)))
        self.nfft, self.hop, self.avg, self.shifted = v[0].value, v[1].value, v[2].value, bool(v[3].value)
        self.window_power = p.value  # sum w[n]^2 in double

    def geometry(self, n_in):
        """(n_seg, n_rows, used_samples) of a call of n_in samples per stream. Host only."""
        return spectrum_geometry(self.nfft, self.hop, self.avg, n_in)

    def work(self, samples):
        """HOST buffer: complex64 [n_streams, n_in] (or a vector: one stream). Returns float32 [n_streams, n_rows, nfft]."""
        x = _complex64(samples, "samples", rows="[n_streams, n_in]")
        n_streams, n_in = x.shape
        rows = self.geometry(n_in)[1] if n_in <= self.max_samples else 0
        out = np.empty((max(n_streams, 1), max(rows, 1), self.nfft), np.float32)
        n = C.c_int()
        check(lib.dvbs2_spectrum_process(self._h, _ptr(x), int(n_in), int(n_in), int(n_streams), out.ctypes.data,
                                         int(max(rows, 1) * self.nfft), C.byref(n)))
        return out[:n_streams, :n.value]

    def work_device(self, d_in, in_stride, n_in, n_streams, d_out, out_stride, stream=0):
        """DEVICE addresses (d_in 8-byte, d_out 4-byte aligned, not overlapping), asynchronous on `stream`: stream i reads n_in complex64
        samples at d_in + 8 * i * in_stride and writes n_rows rows of nfft float32 at d_out + 4 * i * out_stride; out_stride >= n_rows *
        nfft. Returns n_rows (what geometry() said before the call). One call in flight per handle."""
        n = C.c_int()
        check(lib.dvbs2_spectrum_process_device(self._h, d_in or None, int(in_stride), int(n_in), int(n_streams), d_out or None, int(out_stride),
                                                C.byref(n), stream or None))
        return n.value


def pfbch_geometry(n_chan, decim, ntaps):
    """(history in raw samples per stream, delay_num: the delay is delay_num / 2 input samples, taps per branch) (dvbs2_pfbch_geometry).
    Host only."""
    return _ints(3, lib.dvbs2_pfbch_geometry, int(n_chan), int(decim), int(ntaps))


def pfbch_produce(position, decim, n_in):
    """What a call of n_in samples writes per channel when the sample counter stands at `position` (dvbs2_pfbch_produce). Host only."""
    n = lib.dvbs2_pfbch_produce(int(position), int(decim), int(n_in))
    check(min(n, 0))
    return n


def pfbch_check(n_chan, decim, taps, max_streams=1, max_samples=1 << 20):
    """Raises what PfbChannelizer(...) would raise for these arguments, without a device (dvbs2_pfbch_check)."""
    t, t_ptr, ntaps = _f32_vector(taps)
    check(lib.dvbs2_pfbch_check(int(n_chan), int(decim), t_ptr, ntaps, int(max_streams), int(max_samples)))


def pfbch_tile(n_chan, decim, ntaps):
    """Output instants per workgroup of the channelizer's kernel: the tile rule of include/dvbs2_fec_hip.h. Host only."""
    return min(capi.PFBCH_MAX_TILE, (capi.PFBCH_SPAN - (int(ntaps) - 1) - int(n_chan)) // int(decim))


def pfbch_twiddles(n_chan):
    """The transform's one table, complex64 [n_chan / 2] (dvbs2_pfbch_twiddles). Host only."""
    t = np.zeros(max(int(n_chan) // 2, 1), np.complex64)
    check(lib.dvbs2_pfbch_twiddles(int(n_chan), t.ctypes.data))
    return t


class PfbChannelizer(_Handle):
    """A polyphase filter bank channelizer: n_chan equally spaced channels of every input stream, channel c the band centred at
    +c / n_chan of the input rate, each filtered by the caller's real `taps` and output at 1 / decim of the input rate
    (notes/pfbch.md). The last ntaps - 1 raw samples of every stream stay on the device between calls. n samples in give produce(n)
    samples out per selected channel, delayed by delay_num / 2 input samples."""
    _destroy = lib.dvbs2_pfbch_destroy

    def __init__(self, n_chan, decim, taps, max_streams=1, max_samples=1 << 20, device=0):
        t, t_ptr, ntaps = _f32_vector(taps)
        check(lib.dvbs2_pfbch_create(C.byref(self._h), int(n_chan), int(decim), t_ptr, ntaps, int(max_streams), int(max_samples), device))
        self.max_streams, self.max_samples = max_streams, max_samples
        self.n_chan, self.decim, self.ntaps, self.history, self.delay_num, self.tile = _ints(6, lib.dvbs2_pfbch_params, self._h)

    def set_channels(self, channels):
        """From the next call on row i of a stream holds channel channels[i]: 1..n_chan distinct indices in any order. Host only."""
        sel = np.ascontiguousarray(channels, np.int32).reshape(-1)
        check(lib.dvbs2_pfbch_set_channels(self._h, _ptr(sel), int(sel.size)))

    def channels(self):
        """The selection, read back."""
        sel, n = np.zeros(self.n_chan, np.int32), C.c_int()
        check(lib.dvbs2_pfbch_channels(self._h, sel.ctypes.data, C.byref(n)))
        return sel[:n.value].tolist()

    def reset(self):
        check(lib.dvbs2_pfbch_reset(self._h))

    def position(self):
        """The sample counter, from the host's mirror."""
        n = C.c_int64()
        check(lib.dvbs2_pfbch_position(self._h, C.byref(n)))
        return n.value

    def produce(self, n_in):
        """What the next call of n_in samples writes per channel. From the host's mirror: no synchronisation."""
        return pfbch_produce(self.position(), self.decim, n_in)

    def work(self, samples):
        """HOST buffer: complex64 [n_streams, n_in] (or a vector: one stream). Returns complex64 [n_streams, n_sel, produce(n_in)]."""
        x = _complex64(samples, "samples", rows="[n_streams, n_in]")
        n_streams, n_in = x.shape
        n_sel = len(self.channels())
        stride = max(self.produce(n_in), 1) if n_in <= self.max_samples else 1
        out = np.empty((max(n_streams, 1), n_sel, stride), np.complex64)
        n = C.c_int64()
        check(lib.dvbs2_pfbch_process(self._h, _ptr(x), int(n_in), int(n_in), int(n_streams), out.ctypes.data, int(stride), C.byref(n)))
        return out[:n_streams, :, :n.value]

    def work_device(self, d_in, in_stride, n_in, n_streams, d_out, out_stride, stream=0):
        """DEVICE addresses (8-byte aligned, not overlapping), asynchronous on `stream`: stream s reads n_in complex64 samples at
        d_in + 8 * s * in_stride and writes n_out samples of channel channels()[i] at d_out + 8 * (s * n_sel + i) * out_stride;
        out_stride >= n_out. Returns n_out (what produce() said before the call). One call in flight per handle."""
        n = C.c_int64()
        check(lib.dvbs2_pfbch_process_device(self._h, d_in or None, int(in_stride), int(n_in), int(n_streams), d_out or None,
                                             int(out_stride), C.byref(n), stream or None))
        return n.value


def pfbsyn_geometry(n_chan, interp, ntaps):
    """(tail in partial sums per stream, delay_num: the delay is delay_num / 2 OUTPUT samples, taps per phase) (dvbs2_pfbsyn_geometry).
    Host only."""
    return _ints(3, lib.dvbs2_pfbsyn_geometry, int(n_chan), int(interp), int(ntaps))


def pfbsyn_check(n_chan, interp, taps, max_streams=1, max_samples=1 << 20):
    """Raises what PfbSynthesizer(...) would raise for these arguments, without a device (dvbs2_pfbsyn_check)."""
    t, t_ptr, ntaps = _f32_vector(taps)
    check(lib.dvbs2_pfbsyn_check(int(n_chan), int(interp), t_ptr, ntaps, int(max_streams), int(max_samples)))


def pfbsyn_tile(n_chan, interp, ntaps):
    """Input instants per workgroup of the synthesizer's kernel: the tile rule of include/dvbs2_fec_hip.h (dvbs2_pfbsyn_tile; raises for
    a shape that creation refuses). Host only."""
    n = lib.dvbs2_pfbsyn_tile(int(n_chan), int(interp), int(ntaps))
    check(min(n, 0))
    return n


class PfbSynthesizer(_Handle):
    """A polyphase synthesis filter bank, the transpose of PfbChannelizer: the rows of n_chan equally spaced channels become one
    wideband stream at interp times their rate, row i shaped by the caller's real `taps` as an interpolating FIR and moved to
    +channels()[i] / n_chan of the output rate (notes/pfbsyn.md). max(ntaps - interp, 0) partial sums of every stream stay on the
    device between calls. n instants in give n * interp samples out, delayed by delay_num / 2 output samples."""
    _destroy = lib.dvbs2_pfbsyn_destroy

    def __init__(self, n_chan, interp, taps, max_streams=1, max_samples=1 << 20, device=0):
        t, t_ptr, ntaps = _f32_vector(taps)
        check(lib.dvbs2_pfbsyn_create(C.byref(self._h), int(n_chan), int(interp), t_ptr, ntaps, int(max_streams), int(max_samples), device))
        self.max_streams, self.max_samples = max_streams, max_samples
        self.n_chan, self.interp, self.ntaps, self.tail, self.delay_num, self.tile = _ints(6, lib.dvbs2_pfbsyn_params, self._h)

    def set_channels(self, channels):
        """From the next call on row i of a stream feeds channel channels[i]: 1..n_chan distinct indices in any order. Host only."""
        sel = np.ascontiguousarray(channels, np.int32).reshape(-1)
        check(lib.dvbs2_pfbsyn_set_channels(self._h, _ptr(sel), int(sel.size)))

    def channels(self):
        """The selection, read back."""
        sel, n = np.zeros(self.n_chan, np.int32), C.c_int()
        check(lib.dvbs2_pfbsyn_channels(self._h, sel.ctypes.data, C.byref(n)))
        return sel[:n.value].tolist()

    def reset(self):
        check(lib.dvbs2_pfbsyn_reset(self._h))

    def position(self):
        """The counter of input instants, from the host's mirror."""
        n = C.c_int64()
        check(lib.dvbs2_pfbsyn_position(self._h, C.byref(n)))
        return n.value

    def produce(self, n_in):
        """What a call of n_in instants writes per stream: n_in * interp. Host only, no synchronisation."""
        if not 0 <= int(n_in) <= 1 << 24:
            raise ValueError("n_in must be in 0..2^24")
        return int(n_in) * self.interp

    def work(self, samples):
        """HOST buffer: complex64 [n_streams, n_sel, n_in] (or [n_sel, n_in]: one stream). Returns complex64 [n_streams, n_in * interp]."""
        x = np.asarray(samples)
        if x.dtype != np.complex64:
            raise TypeError(f"samples must be complex64, not {x.dtype}")
        if x.ndim == 2:
            x = x.reshape((1,) + x.shape)
        n_sel = len(self.channels())
        if x.ndim != 3 or x.shape[1] != n_sel or not x.flags.c_contiguous:
            raise ValueError("samples must be a C-contiguous [n_streams, n_sel, n_in] or [n_sel, n_in] array")
        n_streams, _, n_in = x.shape
        stride = max(n_in * self.interp, 1)
        out = np.empty((max(n_streams, 1), stride), np.complex64)
        n = C.c_int64()
        check(lib.dvbs2_pfbsyn_process(self._h, _ptr(x), int(n_in), int(n_in), int(n_streams), out.ctypes.data, int(stride), C.byref(n)))
        return out[:n_streams, :n.value]

    def work_device(self, d_in, in_stride, n_in, n_streams, d_out, out_stride, stream=0):
        """DEVICE addresses (8-byte aligned, not overlapping), asynchronous on `stream`: row i of stream s is n_in complex64 samples at
        d_in + 8 * (s * n_sel + i) * in_stride; stream s writes n_in * interp samples at d_out + 8 * s * out_stride; out_stride >= that.
        Returns n_out. One call in flight per handle."""
        n = C.c_int64()
        check(lib.dvbs2_pfbsyn_process_device(self._h, d_in or None, int(in_stride), int(n_in), int(n_streams), d_out or None,
                                              int(out_stride), C.byref(n), stream or None))
        return n.value
