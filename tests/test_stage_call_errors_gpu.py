"""A call that fails leaves its handle as it was: code and text of the failure, then the same answer as a fresh handle.

Every handle type (ldpc, bch, demap, plpayload, plframe, plsync, plcoarse, rotator, symsync, bbdeheader, chain) is created at its smallest
legal size and given one call that fails at an argument check -- inside the stage class where the C ABI reaches one of its texts
(set_expected_pls, the rotator's setters, the LDPC decoder's busy slot), at the entry's own check otherwise. No failure here needs the
device to fault, no buffer is exhausted and no bad device pointer is passed. Each case asserts
  - the code and the exact text of dvbs2_last_error() of the failing call,
  - that a valid call on the same handle then returns DVBS2_OK with outputs equal, byte for byte, to those of the same call on a handle
    that never failed (one such reference per handle type, computed once),
  - what dvbs2_last_error() says after that good call: it is the text of the LAST failed call of the thread, a call that succeeds does
    not clear it -- so it is still the earlier text, for every case.
The codes and texts in CASES were recorded from the library before the stage classes shared a base; one frame (or two samples) per call."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_testlib as T
import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import BbDeheader, BchDecoder, Demapper, FecChain, LdpcDecoder, PlCoarse, PlFrontEnd, PlPayload, PlSync, Rotator, SymbolSync, capi
from dvbs2rx_amd.capi import lib

pytestmark = pytest.mark.gpu

MF = 2  # the smallest max_frames a frame stage takes
SHORT, QPSK = capi.FECFRAME_SHORT, capi.MOD_QPSK
TABLE = "S2_TABLE_C1"  # QPSK 1/4 short
EINVAL, ESIZE, EDEVICE, OK = capi.EINVAL, capi.ESIZE, capi.EDEVICE, capi.OK

TOO_MANY = "n_frames exceeds max_frames"
BAD_PLS = "codeword indexes must be within [0, 128)"


def rng_of(*key):
    return np.random.default_rng([77, *key])


def ptr(a):
    return a.ctypes.data


def cplx(rng, *shape):
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


def blob(*parts):
    """every output of a call as one byte string (arrays by their bytes, anything else by its repr)"""
    return b"|".join(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else repr(a).encode() for a in parts)


ROOM = np.zeros(1 << 16, np.uint8)  # what a refused call is given for a buffer: never read, never written
PLS200 = np.array([3, 200], np.uint8)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


# ------------------------------------------------------------------ per handle type: make(), the good call, the failing calls
def ldpc_make():
    return LdpcDecoder(table=TABLE, message_bits=T.ldpc_info(TABLE)[1], group_size=2, max_frames=MF, max_trials=25)


@functools.lru_cache(None)
def ldpc_llr():
    return T.llr_codeword_awgn(TABLE, 1, 2024, amp=5, sigma=5.6)[0]


def ldpc_good(o):
    bits, llr, ret = o.work(ldpc_llr(), want_llr=True)
    return blob(bits, llr, ret)


def ldpc_busy_slot(o):
    """enqueue, enqueue again before finish(): the second is refused by the decoder object; the first completes with the right answer"""
    import torch
    d_llr = dev(ldpc_llr())
    d_bits, d_out = torch.zeros(o.out_bytes, dtype=torch.uint8, device="cuda"), torch.zeros(o.N, dtype=torch.int8, device="cuda")
    d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (o._h, d_llr.data_ptr(), 1, o.max_trials, o.outputmode, d_bits.data_ptr(), d_out.data_ptr(), d_ret.data_ptr(), T.stream())
    assert lib.dvbs2_ldpc_enqueue_device(*args) == OK
    rc = lib.dvbs2_ldpc_enqueue_device(*args)
    text = lib.dvbs2_last_error()
    assert lib.dvbs2_ldpc_finish(o._h) == OK
    assert blob(d_bits.cpu().numpy(), d_out.cpu().numpy(), d_ret.cpu().numpy()) == reference("ldpc"), "the decode that was in flight"
    assert lib.dvbs2_last_error() == text
    return rc


def bch_make():
    return BchDecoder(framesize=SHORT, rate="C1_4", max_frames=MF)


def bch_good(o):
    cw = np.zeros((1, o.n // 8), np.uint8)
    for pos in rng_of(1).integers(0, o.n, 3):
        cw[0, pos // 8] ^= 0x80 >> (pos % 8)
    return blob(*o.work(cw))


def demap_make():
    return Demapper(framesize=SHORT, rate="C1_4", constellation=QPSK, max_frames=MF)


def demap_good(o):
    return blob(o.work(cplx(rng_of(2), 1, o.n_syms), np.float32(0.3)))


def plpayload_make():
    return PlPayload(gold_code=0, n_slots=36, has_pilots=True, max_frames=MF)


def plpayload_good(o):
    rng = rng_of(3)
    return blob(o.work(cplx(rng, 1, o.payload_len), [0.4], [1e-4], [1], rng.uniform(-3, 3, (1, max(o.n_pilots, 1)))))


def plframe_make():
    return PlFrontEnd(gold_code=0, plsc=P.SHORT_QPSK, max_frames=MF)


def plframe_good(o):
    frames, _ = M.make_plframes(P.SHORT_QPSK, 0, 1, rng_of(4), es_n0_db=8.0, phase=0.3, foffset=1e-4)
    out, est = o.work(np.ascontiguousarray(frames.reshape(1, o.plframe_len), np.complex64), np.ones(1, np.int32))
    return blob(out, *[est[k] for k, _ in PlFrontEnd.EST])


def plsync_make():
    return PlSync(plsc=-1, max_symbols=PlSync.MIN_SYMBOLS, max_frames=MF)


def plsync_good(o):
    x = P.make_stream([P.SHORT_QPSK, P.SHORT_QPSK], 7, offset=500)[0]
    assert x.size <= PlSync.MIN_SYMBOLS
    recs, consumed, state = o.work(x)
    assert len(recs) > 0
    return blob(recs, consumed, state)


def plcoarse_make():
    return PlCoarse(period=1, plsc=-1, max_frames=MF)


def plcoarse_good(o):
    x = (M.plheader(P.SHORT_QPSK) * np.exp(2j * np.pi * 0.01 * np.arange(90))).astype(np.complex64).reshape(1, 90)
    r = o.work(x, [P.SHORT_QPSK])
    return blob(r["coarse_foffset"], r["coarse_corrected"], r["new_est"])


def rotator_good(o):
    return blob(o.work(P.qpsk(rng_of(8), 64).astype(np.complex64)), o.position())


def symsync_make():
    return SymbolSync(sps=2, max_streams=1, max_samples=2)


def symsync_good(o):
    syms, idx, mu, consumed, status = o.work(cplx(rng_of(9), 2))
    return blob(syms, idx, mu, consumed, status, sorted(o.state().items()))


def bbdeheader_make():
    return BbDeheader(framesize=SHORT, rate="C1_4", max_frames=MF)


def bbdeheader_good(o):
    kbch = o.kbch_bytes * 8
    frames = T.bbframe_stream(kbch, 1, T.ts_up_stream(-(-(kbch - 80) // (8 * 188)), rng_of(6)), 0)
    return blob(o.work(frames[:1]), sorted(o.counters().items()))


def chain_make():
    return FecChain(framesize=SHORT, rate="C1_4", constellation=QPSK, group_size=2, max_frames=MF, max_trials=25)


@functools.lru_cache(None)
def chain_syms():
    return cplx(rng_of(10), 1, 8100)


def chain_good(o):
    assert o.n_syms == chain_syms().shape[1]
    return blob(*o.work(chain_syms(), np.float32(0.5)))


def chain_pending(o):
    """enqueue, enqueue again before finish(): refused by the chain's own flag; the first completes with the right answer"""
    import torch
    d_syms, d_n0 = dev(chain_syms()), dev(np.array([0.5], np.float32))
    d_msg = torch.zeros(o.msg_bytes, dtype=torch.uint8, device="cuda")
    d_ret, d_corr = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (o._h, d_syms.data_ptr(), 1, d_n0.data_ptr(), 1, o.max_trials, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr(), T.stream())
    assert lib.dvbs2_chain_enqueue_device(*args) == OK
    rc = lib.dvbs2_chain_enqueue_device(*args)
    text = lib.dvbs2_last_error()
    assert lib.dvbs2_chain_finish(o._h) == OK
    assert blob(d_msg.cpu().numpy(), d_ret.cpu().numpy(), d_corr.cpu().numpy()) == reference("chain"), "the decode that was in flight"
    assert lib.dvbs2_last_error() == text
    return rc


R = ptr(ROOM)
STAGES = {  # name -> (make, good)
    "ldpc": (ldpc_make, ldpc_good), "bch": (bch_make, bch_good), "demap": (demap_make, demap_good),
    "plpayload": (plpayload_make, plpayload_good), "plframe": (plframe_make, plframe_good), "plsync": (plsync_make, plsync_good),
    "plcoarse": (plcoarse_make, plcoarse_good), "rotator": (lambda: Rotator(phase_inc=0.01), rotator_good),
    "symsync": (symsync_make, symsync_good), "bbdeheader": (bbdeheader_make, bbdeheader_good), "chain": (chain_make, chain_good),
}
EST = capi.PlFrameEstimates()
CASES = [  # (handle type, what fails, the failing call -> code, expected code, expected text)
    ("ldpc", "frames", lambda o: lib.dvbs2_ldpc_decode(o._h, R, MF + 1, 25, capi.OM_MESSAGE, R, None, None), ESIZE, TOO_MANY),
    ("ldpc", "frames_device", lambda o: lib.dvbs2_ldpc_decode_device(o._h, R, MF + 1, 25, capi.OM_MESSAGE, R, None, None, None), ESIZE, TOO_MANY),
    ("ldpc", "busy_slot", ldpc_busy_slot, EDEVICE, "slot busy: finish() the previous decode first"),
    ("bch", "frames", lambda o: lib.dvbs2_bch_decode(o._h, R, MF + 1, R, R), ESIZE, TOO_MANY),
    ("bch", "frames_device", lambda o: lib.dvbs2_bch_decode_device(o._h, R, MF + 1, R, R, None), ESIZE, TOO_MANY),
    ("demap", "frames", lambda o: lib.dvbs2_demap_soft(o._h, R, MF + 1, R, 1, R), ESIZE, TOO_MANY),
    ("demap", "snr_frames", lambda o: lib.dvbs2_demap_estimate_snr(o._h, R, MF + 1, R), ESIZE, TOO_MANY),
    ("plpayload", "frames", lambda o: lib.dvbs2_plpayload_process(o._h, R, MF + 1, R, R, R, R, R), ESIZE, TOO_MANY),
    ("plframe", "expected_pls", lambda o: lib.dvbs2_plframe_set_expected_pls(o._h, ptr(PLS200), 2), EINVAL, BAD_PLS),
    ("plframe", "frames", lambda o: lib.dvbs2_plframe_process(o._h, R, MF + 1, 0, R, None, R, C.byref(EST)), ESIZE, TOO_MANY),
    ("plsync", "expected_pls", lambda o: lib.dvbs2_plsync_set_expected_pls(o._h, ptr(PLS200), 2), EINVAL, BAD_PLS),
    ("plsync", "symbols", lambda o: lib.dvbs2_plsync_search(o._h, R, PlSync.MIN_SYMBOLS + 1, R, None, None, None), ESIZE, "n_syms exceeds max_symbols"),
    ("plsync", "symbols_device", lambda o: lib.dvbs2_plsync_search_device(o._h, R, PlSync.MIN_SYMBOLS + 1, R, None), ESIZE, "n_syms exceeds max_symbols"),
    ("plsync", "gather_frames", lambda o: lib.dvbs2_plsync_gather_device(o._h, R, R, MF + 1, P.SHORT_QPSK, R, R, None), ESIZE, TOO_MANY),
    ("plcoarse", "frames", lambda o: lib.dvbs2_plcoarse_estimate(o._h, R, 90, R, MF + 1, R, R, R), ESIZE, TOO_MANY),
    ("plcoarse", "stride", lambda o: lib.dvbs2_plcoarse_estimate(o._h, R, 89, R, 1, R, R, R), EINVAL, "stride below the 90 header symbols"),
    ("plcoarse", "stride_device", lambda o: lib.dvbs2_plcoarse_estimate_device(o._h, R, 89, R, 1, R, R, R, None), EINVAL, "stride below the 90 header symbols"),
    ("plcoarse", "no_plsc", lambda o: lib.dvbs2_plcoarse_estimate(o._h, R, 90, None, 1, R, R, R), EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array"),
    ("plcoarse", "no_plsc_device", lambda o: lib.dvbs2_plcoarse_estimate_device(o._h, R, 90, None, 1, R, R, R, None), EINVAL,
     "a handle without a fixed PLSC needs the per-frame PLSC array"),
    ("rotator", "phase_inc", lambda o: lib.dvbs2_rotator_set_phase_inc(o._h, float("nan")), EINVAL, "phase_inc must be finite"),
    ("rotator", "schedule_offset", lambda o: lib.dvbs2_rotator_schedule(o._h, -1, 0.1), EINVAL, "offset must not be negative"),
    ("rotator", "seek", lambda o: lib.dvbs2_rotator_seek(o._h, -1), EINVAL, "seek distance out of range"),
    ("rotator", "alignment", lambda o: lib.dvbs2_rotator_rotate_device(o._h, R + 4, 1, R, None), EINVAL, "symbol buffers must be 8-byte aligned"),
    ("symsync", "samples", lambda o: lib.dvbs2_symsync_work(o._h, R, 3, R, 3, None, None, None, None, None), ESIZE, "n_in exceeds max_samples"),
    ("symsync", "streams", lambda o: lib.dvbs2_symsync_work_device(o._h, R, 2, ptr(np.array([2, 2], np.int32)), 2, R, 2, 2, None, None, None), ESIZE,
     "n_streams exceeds max_streams"),
    ("bbdeheader", "frames", lambda o: lib.dvbs2_bbdeheader_process(o._h, R, MF + 1, R, None), ESIZE, TOO_MANY),
    ("chain", "frames", lambda o: lib.dvbs2_chain_decode(o._h, R, MF + 1, R, 1, 25, R, None, None), ESIZE, TOO_MANY),
    ("chain", "pending", chain_pending, EINVAL, "previous call not finished"),
]


@functools.lru_cache(None)
def reference(stage):
    """the good call on a handle that never failed"""
    make, good = STAGES[stage]
    o = make()
    out = good(o)
    o.close()
    return out


def test_every_handle_type_has_a_case():
    assert {c[0] for c in CASES} == set(STAGES)
    assert ROOM.ctypes.data % 8 == 0


@pytest.mark.parametrize("stage,what,bad,code,text", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_failed_call_leaves_the_handle_usable(stage, what, bad, code, text):
    make, good = STAGES[stage]
    want = reference(stage)
    o = make()
    rc = bad(o)
    got_text = lib.dvbs2_last_error().decode()
    print(f"{stage}-{what}: code {rc} text {got_text!r}")
    assert (rc, got_text) == (code, text)
    assert not ROOM.any(), "a refused call wrote to a buffer"
    assert good(o) == want, "after the failed call the handle answers differently from a fresh one"
    assert lib.dvbs2_last_error().decode() == text  # the last ERROR: a call that succeeds does not clear it
    o.close()
