"""Pulse shaper on the device (dvbs2_pulse_*) against the float32 model (a) of tests/pulse_model.py: every output sample BIT FOR BIT
(uint32 compare) into sentinel-filled buffers whose pads and gaps must stay untouched, with zeros of both signs and denormals planted
in the input; then the receive stages of this library in a closed loop on what it wrote. The model runs on the taps the library
designed (pulse_taps), so the comparison does not depend on libm."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import pulse_model as PM
from dvbs2rx_amd import PulseShaper, capi, pulse_geometry, pulse_taps
from fec_testlib import PAD, SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu

K = capi.PULSE_TILE    # the kernel's tile in symbols


def shape_on_device(ps, xs, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the streams xs (complex64 vectors of one length n) through fec_testlib.run_strided: stream s lies at
    in_shift + s * in_stride complex elements of the input buffer and writes at out_shift + s * out_stride of a sentinel buffer. Returns one
    uint32 (n * sps, 2) array per stream."""
    ns, n = len(xs), xs[0].size
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(n * ps.sps, 1) if out_stride is None else out_stride
    return T.run_strided(lambda a, o: ps.work_device(a, in_stride, n, ns, o, out_stride, stream()), xs, [n * ps.sps] * ns, in_stride, out_stride,
                         in_shift, out_shift)[0]


def same(got, want, what):
    T.same_bits(got, PM.bits(want), what)


@functools.lru_cache(maxsize=None)
def data(seed, n):
    x = PM.planted(np.random.default_rng(seed), n)
    x.setflags(write=False)
    return x


def sizes(history):
    return sorted({n for n in (1, history - 1, history, history + 1, K - 1, K, K + 1, 3 * K + 7) if n >= 1})


# ------------------------------------------------------------------ 1. designed taps
@pytest.mark.parametrize("sps,delay", [(2, 1), (2, 5), (4, 5), (6, 3)])
def test_designed_taps_equal_the_model(sps, delay):
    """(6, 3) has three lanes per symbol. Each size runs from a reset handle, then a second call continues from its history."""
    taps = pulse_taps(sps, 0.2, delay)
    ps = PulseShaper(sps, 0.2, delay, max_symbols=3 * K + 7)
    assert (ps.sps, ps.ntaps, ps.history, ps.delay) == (sps, *pulse_geometry(sps, delay)) and ps.history == 2 * delay
    for n in sizes(ps.history):
        ps.reset()
        x, more = data(sps * 100 + delay, 3 * K + 7)[:n], data(7, 40)
        want, hist = PM.shape32(taps, sps, x)
        same(shape_on_device(ps, [x])[0], want, f"sps {sps} delay {delay}: {n} symbols")
        same(shape_on_device(ps, [more])[0], PM.shape32(taps, sps, more, hist)[0], f"sps {sps} delay {delay}: 40 symbols behind {n}")
    ps.close()


# ------------------------------------------------------------------ 2. a caller's taps, ragged phases
@pytest.mark.parametrize("sps,ntaps", [(2, 8), (4, 7), (4, 1), (2, 258)])
def test_callers_taps_with_ragged_phases(sps, ntaps):
    """ntaps that is no multiple of sps + 1: the phases have different numbers of terms, (4, 1) has phases without any (their samples
    are +0.0) and no history, (2, 258) the 129 terms and the 128 symbols of history that are the cap."""
    rng = np.random.default_rng(ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    ps = PulseShaper(sps, taps=taps, max_symbols=2 * K + 5)
    H = PM.history_of(ntaps, sps)
    assert (ps.ntaps, ps.history, ps.delay) == (ntaps, H, (ntaps - 1) // 2)
    for n in sorted({1, H + 1, K + 1, 2 * K + 5}):
        ps.reset()
        x, more = data(50 + ntaps, 2 * K + 5)[:n], data(8, 33)
        want, hist = PM.shape32(taps, sps, x)
        got = shape_on_device(ps, [x])[0]
        same(got, want, f"sps {sps} ntaps {ntaps}: {n} symbols")
        if ntaps < sps:
            assert (got.reshape(n, sps, 2)[:, ntaps:] == 0).all()  # +0.0, not -0.0
        same(shape_on_device(ps, [more])[0], PM.shape32(taps, sps, more, hist)[0], f"sps {sps} ntaps {ntaps}: 33 symbols behind {n}")
    ps.close()


# ------------------------------------------------------------------ 3. streams
@pytest.mark.parametrize("sps,pad_out", [(2, 5), (4, 6)])
def test_streams_keep_their_own_history(sps, pad_out):
    """3 streams with strides larger than the data; an odd output stride (sps 2) takes the 8-byte stores, an even one the 16-byte ones."""
    taps = pulse_taps(sps, 0.2, 5)
    ps = PulseShaper(sps, 0.2, 5, max_streams=3, max_symbols=K + 9)
    n1, n2 = K + 9, 7  # the second call is shorter than the history: old history and input both enter the new one
    first = [data(20 + s, n1) for s in range(3)]
    second = [data(30 + s, n2) for s in range(3)]
    got = shape_on_device(ps, first, in_stride=n1 + 3, out_stride=n1 * sps + pad_out)
    hists = []
    for s in range(3):
        want, h = PM.shape32(taps, sps, first[s])
        same(got[s], want, f"stream {s}, first call")
        hists.append(h)
    got = shape_on_device(ps, second, in_stride=n2 + 1, out_stride=n2 * sps + pad_out)
    for s in range(3):
        want, hists[s] = PM.shape32(taps, sps, second[s], hists[s])
        same(got[s], want, f"stream {s}, second call")
    # two streams only: stream 2 keeps what it had
    got = shape_on_device(ps, second[:2], in_stride=n2, out_stride=n2 * sps)
    for s in range(2):
        want, hists[s] = PM.shape32(taps, sps, second[s], hists[s])
        same(got[s], want, f"stream {s}, third call")
    got = shape_on_device(ps, first, in_stride=n1, out_stride=n1 * sps)
    for s in range(3):
        same(got[s], PM.shape32(taps, sps, first[s], hists[s])[0], f"stream {s}, fourth call")
    ps.close()


# ------------------------------------------------------------------ 4. pieces
@pytest.mark.parametrize("sps,delay", [(2, 5), (4, 5)])
def test_pieces_give_the_bits_of_one_call(sps, delay):
    taps = pulse_taps(sps, 0.2, delay)
    n = 2 * K + 61
    ps = PulseShaper(sps, 0.2, delay, max_symbols=n)
    x = data(40 + sps, n)
    whole = shape_on_device(ps, [x])[0]
    same(whole, PM.shape32(taps, sps, x)[0], "one call")
    ps.reset()
    H = ps.history
    cuts = [1, 0, H - 1, 2, K + 3]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    parts, pos = [], 0
    for c in cuts:
        parts.append(shape_on_device(ps, [x[pos:pos + c]])[0])
        pos += c
    assert np.array_equal(np.concatenate(parts), whole), cuts
    ps.reset()  # the first-call result again
    assert np.array_equal(shape_on_device(ps, [x])[0], whole)
    ps.close()


# ------------------------------------------------------------------ 5. alignment
@pytest.mark.parametrize("sps", [2, 4])
@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_alignment(sps, in_shift, out_shift):
    """Buffers displaced by one complex element are 8-byte but not 16-byte aligned: the same bits."""
    taps = pulse_taps(sps, 0.2, 5)
    ps = PulseShaper(sps, 0.2, 5, max_symbols=K + 7)
    x = data(60, K + 7)
    same(shape_on_device(ps, [x], in_shift=in_shift, out_shift=out_shift)[0], PM.shape32(taps, sps, x)[0], f"shifts {in_shift} {out_shift}")
    ps.close()


# ------------------------------------------------------------------ 6. the host entry
def test_host_entry_equals_the_device_entry():
    taps = pulse_taps(4, 0.35, 3, 0.25)
    a, b = PulseShaper(4, taps=taps, max_symbols=K + 30), PulseShaper(4, taps=taps, max_symbols=K + 30)
    hist = None
    for n in (K + 30, 3, 0, 50):
        x = data(70 + n, max(n, 1))[:n]
        got = a.work(x)
        want, hist = PM.shape32(taps, 4, x, hist)
        assert got.dtype == np.complex64 and got.size == n * 4
        same(PM.bits(got).reshape(-1, 2), want, f"host entry, {n} symbols")
        if n:
            assert np.array_equal(shape_on_device(b, [x])[0], PM.bits(got).reshape(-1, 2))
    a.close()
    b.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_history_and_output_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    # creation (the same answers without a device: tests/test_pulse_model.py)
    good_taps = np.ones(21, np.float32)
    inf_taps = good_taps.copy()
    inf_taps[4] = -np.inf
    refused(capi.EINVAL, "sps must be an even integer in 2..64, rrc_delay in 1..64", lib.dvbs2_pulse_create, C.byref(h), 3, 0.2, 5, 1, 16, 0)
    refused(capi.EINVAL, "sps must be an even integer in 2..64, rrc_delay in 1..64", lib.dvbs2_pulse_create, C.byref(h), 2, 0.2, 0, 1, 16, 0)
    refused(capi.EINVAL, "rolloff must lie in [0, 1]", lib.dvbs2_pulse_create, C.byref(h), 2, -0.2, 5, 1, 16, 0)
    refused(capi.EINVAL, "max_streams out of range (1..65535: streams are one launch dimension)", lib.dvbs2_pulse_create, C.byref(h), 2, 0.2, 5, 0, 16, 0)
    refused(capi.EINVAL, "max_symbols out of range (1..2^30)", lib.dvbs2_pulse_create, C.byref(h), 2, 0.2, 5, 1, 0, 0)
    refused(capi.EINVAL, "taps[4] is not finite", lib.dvbs2_pulse_create_taps, C.byref(h), 2, inf_taps.ctypes.data, 21, 1, 16, 0)
    refused(capi.EINVAL, "null taps", lib.dvbs2_pulse_create_taps, C.byref(h), 2, None, 21, 1, 16, 0)
    refused(capi.EINVAL, "ntaps must be at least 1 and at most 129 taps per phase (ceil(ntaps / sps) <= 129)", lib.dvbs2_pulse_create_taps,
            C.byref(h), 2, good_taps.ctypes.data, 0, 1, 16, 0)
    refused(capi.EINVAL, "sps must be an even integer in 2..64", lib.dvbs2_pulse_create_taps, C.byref(h), 7, good_taps.ctypes.data, 21, 1, 16, 0)
    refused(capi.EINVAL, "null handle pointer", lib.dvbs2_pulse_create, None, 2, 0.2, 5, 1, 16, 0)
    assert not h
    assert lib.dvbs2_pulse_create(C.byref(h), 2, 0.2, 5, 1, 16, 99) < 0 and not h  # no such device

    sps, n = 2, 100
    taps = pulse_taps(sps, 0.2, 5)
    ps = PulseShaper(sps, 0.2, 5, max_streams=2, max_symbols=n)
    first, second = [data(80 + s, n) for s in range(2)], [data(90 + s, n) for s in range(2)]
    got = shape_on_device(ps, first)
    hists = [PM.shape32(taps, sps, first[s])[1] for s in range(2)]
    d_in = torch.from_numpy(np.concatenate(second).view(np.float32)).cuda()
    d_out = sentinel(2 * (2 * n * sps + PAD))
    st = stream()
    a, o = d_in.data_ptr(), d_out.data_ptr()
    entry = lib.dvbs2_pulse_shape_device
    refused(capi.ESIZE, "n_syms exceeds max_symbols", entry, ps._h, a, n, n + 1, 1, o, n * sps, st)
    refused(capi.ESIZE, "n_streams exceeds max_streams", entry, ps._h, a, n, n, 3, o, n * sps, st)
    refused(capi.EINVAL, "in_stride is below n_syms", entry, ps._h, a, n - 1, n, 2, o, n * sps, st)
    refused(capi.EINVAL, "out_stride is below n_syms * sps", entry, ps._h, a, n, n, 2, o, n * sps - 1, st)
    refused(capi.EINVAL, "in is null", entry, ps._h, None, n, n, 2, o, n * sps, st)
    refused(capi.EINVAL, "out is null", entry, ps._h, a, n, n, 2, None, n * sps, st)
    refused(capi.EINVAL, "n_syms is negative", entry, ps._h, a, n, -1, 2, o, n * sps, st)
    refused(capi.EINVAL, "n_streams is negative", entry, ps._h, a, n, n, -1, o, n * sps, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, ps._h, a + 4, n, n, 2, o, n * sps, st)
    assert entry(ps._h, None, 0, 0, 2, None, 0, st) == capi.OK  # n_syms == 0: a successful call that does nothing
    assert entry(ps._h, a, 0, 0, 2, o, 0, st) == capi.OK
    assert entry(ps._h, a, 0, n, 1, o, 0, st) == capi.OK  # one stream: the strides do not matter (this call is the good one below, on stream 0)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    want0, hists[0] = PM.shape32(taps, sps, second[0], hists[0])
    same(out[:n * sps], want0, "the one-stream call behind the refusals")
    assert (out[n * sps:] == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = second[0].copy(), np.zeros(n * sps, np.complex64)
    refused(capi.ESIZE, "n_syms exceeds max_symbols", lib.dvbs2_pulse_shape, ps._h, host_in.ctypes.data, n + 1, host_out.ctypes.data)
    refused(capi.EINVAL, "n_syms is negative", lib.dvbs2_pulse_shape, ps._h, host_in.ctypes.data, -1, host_out.ctypes.data)
    refused(capi.EINVAL, "in is null", lib.dvbs2_pulse_shape, ps._h, None, n, host_out.ctypes.data)
    refused(capi.EINVAL, "out is null", lib.dvbs2_pulse_shape, ps._h, host_in.ctypes.data, n, None)
    assert lib.dvbs2_pulse_shape(ps._h, None, 0, None) == capi.OK
    assert (host_out == 0).all()
    # no refusal touched a history: both streams go on from where the good calls left them
    got = shape_on_device(ps, first)
    for s in range(2):
        same(got[s], PM.shape32(taps, sps, first[s], hists[s])[0], f"stream {s} behind the refusals")
    ps.close()


# ------------------------------------------------------------------ 8. closed loop through the receiver, noise-free
def test_closed_loop_through_the_receiver():
    """loopback.shaped_six_frames is this stage in the loop: the encoder's frames behind an odd lead through the shaper, its taps through
    create_taps, shifted by 0.3 symbols and scaled for unit symbols behind the receiver's matched filter."""
    seq, plsc, nd, lead = L.SEQ6, L.PLSC, 6, 301
    tx = L.shaped_six_frames(lead, seed=2026)
    rx = L.timing_and_frames(tx.d_y, tx.ns, L.SPS, L.ROLLOFF, 0, tx.n_all, tol=12)
    recs = rx.recs
    assert rx.state == capi.PLSYNC_LOCKED and rx.nf == len(seq) and recs["plsc"].tolist() == seq  # every frame found
    shifts = set((recs["sof_index"] - (lead + tx.lay["out_offset"])).tolist())
    assert len(shifts) == 1, shifts  # one constant delay
    shift = shifts.pop()
    print(f"closed loop: {rx.nsym} symbols from {tx.ns} samples, SOF shift {shift} symbols (shaper delay {L.RRC_DELAY})")
    assert abs(shift - L.RRC_DELAY) <= 12  # the loop's start-up and the matched filter, moved by this stage's own delay in symbols
    got = L.decode_frames(rx, plsc, L.GOLD, 0.02)
    assert len(got.locked) >= nd - 1  # the tracker locks at the second header
    assert np.array_equal(got.msg, tx.sent[got.data_index])  # the encoder's input bytes
    rx.sync.close()
