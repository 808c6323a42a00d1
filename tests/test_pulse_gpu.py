"""Pulse shaper on the device (dvbs2_pulse_*) against the float32 model (a) of tests/pulse_model.py: every output sample BIT FOR BIT
(uint32 compare) into sentinel-filled buffers whose pads and gaps must stay untouched, with zeros of both signs and denormals planted
in the input; then the receive stages of this library in a closed loop on what it wrote. The model runs on the taps the library
designed (pulse_taps), so the comparison does not depend on libm."""
import ctypes as C
import functools

import numpy as np
import pytest

import plframe_model as M
import plsync_model as P
import pulse_model as PM
from dvbs2rx_amd import (FecChain, FecEncoder, PlCoarse, PlFramer, PlFrontEnd, PlSync, PulseShaper, SymbolSync, capi, plframer_layout,
                         pulse_geometry, pulse_taps, symsync_taps)

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3A55A3C  # a bit pattern no output of these tests holds
PAD = 64               # sentinel samples behind each stream's output
K = capi.PULSE_TILE    # the kernel's tile in symbols


def _torch():
    import torch
    return torch


def stream():
    return _torch().cuda.current_stream().cuda_stream


def sentinel(n_elems):
    """n_elems complex elements of the sentinel, as int32 (torch has no uint32 arithmetic worth the name)"""
    torch = _torch()
    return torch.full((n_elems * 2,), np.uint32(SENTINEL).astype(np.int32).item(), dtype=torch.int32, device="cuda")


def shape_on_device(ps, xs, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the streams xs (complex64 vectors of one length n). Stream s lies at in_shift + s * in_stride complex
    elements of a 16-byte-aligned input buffer and writes at out_shift + s * out_stride of a 16-byte-aligned sentinel buffer. Returns one
    uint32 (n * sps, 2) array per stream after checking that everything else in the output buffer -- the shift in front, the gaps between the
    streams and PAD elements behind the last -- is still the sentinel, and that the input is unchanged."""
    torch = _torch()
    ns, n = len(xs), xs[0].size
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(n * ps.sps, 1) if out_stride is None else out_stride
    host_in = np.full(in_shift + ns * in_stride + 2, np.complex64(complex(9.5, -9.5)), np.complex64)
    for s, x in enumerate(xs):
        assert x.size == n
        host_in[in_shift + s * in_stride:in_shift + s * in_stride + n] = x
    d_in = torch.from_numpy(host_in.view(np.float32)).cuda()
    n_out = out_shift + (ns - 1) * out_stride + n * ps.sps + PAD
    d_out = sentinel(n_out)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    ps.work_device(d_in.data_ptr() + 8 * in_shift, in_stride, n, ns, d_out.data_ptr() + 8 * out_shift, out_stride, stream())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), host_in.view(np.uint32))
    touched = np.zeros(n_out, bool)
    outs = []
    for s in range(ns):
        a = out_shift + s * out_stride
        touched[a:a + n * ps.sps] = True
        outs.append(got[a:a + n * ps.sps])
    assert (got[~touched] == SENTINEL).all(), "a write outside the streams' outputs"
    return outs


def same(got, want, what):
    assert got.shape[0] == want.size, what
    w = PM.bits(want).reshape(-1, 2)
    if not np.array_equal(got, w):
        bad = np.nonzero((got != w).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {want.size} samples differ, the first at {bad[0]}: {got[bad[0]]} != {w[bad[0]]}")


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
def _refused(code, text, entry, *args):
    assert entry(*args) == code, (entry.__name__, capi.lib.dvbs2_last_error())
    assert capi.lib.dvbs2_last_error() == text.encode(), capi.lib.dvbs2_last_error()


def test_refusals_leave_history_and_output_untouched():
    torch = _torch()
    lib, h = capi.lib, C.c_void_p()
    # creation (the same answers without a device: tests/test_pulse_model.py)
    good_taps = np.ones(21, np.float32)
    inf_taps = good_taps.copy()
    inf_taps[4] = -np.inf
    _refused(capi.EINVAL, "sps must be an even integer in 2..64, rrc_delay in 1..64", lib.dvbs2_pulse_create, C.byref(h), 3, 0.2, 5, 1, 16, 0)
    _refused(capi.EINVAL, "sps must be an even integer in 2..64, rrc_delay in 1..64", lib.dvbs2_pulse_create, C.byref(h), 2, 0.2, 0, 1, 16, 0)
    _refused(capi.EINVAL, "rolloff must lie in [0, 1]", lib.dvbs2_pulse_create, C.byref(h), 2, -0.2, 5, 1, 16, 0)
    _refused(capi.EINVAL, "max_streams out of range (1..65535: streams are one launch dimension)", lib.dvbs2_pulse_create, C.byref(h), 2, 0.2, 5, 0, 16, 0)
    _refused(capi.EINVAL, "max_symbols out of range (1..2^30)", lib.dvbs2_pulse_create, C.byref(h), 2, 0.2, 5, 1, 0, 0)
    _refused(capi.EINVAL, "taps[4] is not finite", lib.dvbs2_pulse_create_taps, C.byref(h), 2, inf_taps.ctypes.data, 21, 1, 16, 0)
    _refused(capi.EINVAL, "null taps", lib.dvbs2_pulse_create_taps, C.byref(h), 2, None, 21, 1, 16, 0)
    _refused(capi.EINVAL, "ntaps must be at least 1 and at most 129 taps per phase (ceil(ntaps / sps) <= 129)", lib.dvbs2_pulse_create_taps,
             C.byref(h), 2, good_taps.ctypes.data, 0, 1, 16, 0)
    _refused(capi.EINVAL, "sps must be an even integer in 2..64", lib.dvbs2_pulse_create_taps, C.byref(h), 7, good_taps.ctypes.data, 21, 1, 16, 0)
    _refused(capi.EINVAL, "null handle pointer", lib.dvbs2_pulse_create, None, 2, 0.2, 5, 1, 16, 0)
    assert not h
    assert lib.dvbs2_pulse_create(C.byref(h), 2, 0.2, 5, 1, 16, 99) < 0 and not h  # no such device

    sps, n = 2, 100
    taps = pulse_taps(sps, 0.2, 5)
    ps = PulseShaper(sps, 0.2, 5, max_streams=2, max_symbols=n)
    first, second = [data(80 + s, n) for s in range(2)], [data(90 + s, n) for s in range(2)]
    got = shape_on_device(ps, first)
    hists = [PM.shape32(taps, sps, first[s])[1] for s in range(2)]
    d_in = torch.from_numpy(np.concatenate(second).view(np.float32)).cuda()
    d_out = sentinel(2 * n * sps + PAD)
    st = stream()
    a, o = d_in.data_ptr(), d_out.data_ptr()
    entry = lib.dvbs2_pulse_shape_device
    _refused(capi.ESIZE, "n_syms exceeds max_symbols", entry, ps._h, a, n, n + 1, 1, o, n * sps, st)
    _refused(capi.ESIZE, "n_streams exceeds max_streams", entry, ps._h, a, n, n, 3, o, n * sps, st)
    _refused(capi.EINVAL, "in_stride is below n_syms", entry, ps._h, a, n - 1, n, 2, o, n * sps, st)
    _refused(capi.EINVAL, "out_stride is below n_syms * sps", entry, ps._h, a, n, n, 2, o, n * sps - 1, st)
    _refused(capi.EINVAL, "in is null", entry, ps._h, None, n, n, 2, o, n * sps, st)
    _refused(capi.EINVAL, "out is null", entry, ps._h, a, n, n, 2, None, n * sps, st)
    _refused(capi.EINVAL, "n_syms is negative", entry, ps._h, a, n, -1, 2, o, n * sps, st)
    _refused(capi.EINVAL, "n_streams is negative", entry, ps._h, a, n, n, -1, o, n * sps, st)
    _refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, ps._h, a + 4, n, n, 2, o, n * sps, st)
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
    _refused(capi.ESIZE, "n_syms exceeds max_symbols", lib.dvbs2_pulse_shape, ps._h, host_in.ctypes.data, n + 1, host_out.ctypes.data)
    _refused(capi.EINVAL, "n_syms is negative", lib.dvbs2_pulse_shape, ps._h, host_in.ctypes.data, -1, host_out.ctypes.data)
    _refused(capi.EINVAL, "in is null", lib.dvbs2_pulse_shape, ps._h, None, n, host_out.ctypes.data)
    _refused(capi.EINVAL, "out is null", lib.dvbs2_pulse_shape, ps._h, host_in.ctypes.data, n, None)
    assert lib.dvbs2_pulse_shape(ps._h, None, 0, None) == capi.OK
    assert (host_out == 0).all()
    # no refusal touched a history: both streams go on from where the good calls left them
    got = shape_on_device(ps, first)
    for s in range(2):
        same(got[s], PM.shape32(taps, sps, first[s], hists[s])[0], f"stream {s} behind the refusals")
    ps.close()


# ------------------------------------------------------------------ 8. closed loop through the receiver, noise-free
def test_closed_loop_through_the_receiver():
    torch = _torch()
    sps, rolloff, rrc_delay, tau = 2, 0.2, 5, 0.3
    gold, plsc, dummy, nd = 5, P.plsc_of(1, 1, 1), P.plsc_of(0, 0, 0), 6
    rng = np.random.default_rng(2026)
    st = stream()
    # transmit: encoder, PL framer behind an odd lead of random symbols, shaper
    enc = FecEncoder(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, max_frames=nd)
    enc.set_scramble(True)
    sent = rng.integers(0, 256, (nd, enc.in_bytes), dtype=np.uint8)
    seq = [plsc, plsc, dummy, plsc, plsc, dummy, plsc, plsc]  # a dummy frame after data frames 2 and 4
    lay = plframer_layout(seq)
    L = M.pls_parse(plsc)["plframe_len"]
    assert enc.n_syms == M.pls_parse(plsc)["xfecframe_len"] and lay["in_syms"] == nd * enc.n_syms
    d_xfec = torch.zeros((nd, enc.n_syms, 2), dtype=torch.float32, device="cuda")
    enc.work_device(torch.from_numpy(sent).cuda().data_ptr(), nd, d_syms=d_xfec.data_ptr(), stream=st)
    fr = PlFramer(gold, max_frames=len(seq))
    fr.set_sequence(seq)
    # the taps go in through create_taps: the library's design shifted by tau, scaled so that the centre of the convolution of the
    # UNSHIFTED design with subfilter 0 of the receiver's bank (its matched filter at mu = 0) is 1 -- unit symbol amplitude behind the
    # matched filter at the right instant; the shift moves the pulse and leaves its scale alone
    bank0 = symsync_taps(sps, rolloff, rrc_delay, 128)[0].astype(np.float64)[::-1]  # the bank holds each subfilter flipped
    centre = np.convolve(pulse_taps(sps, rolloff, rrc_delay).astype(np.float64), bank0)[2 * sps * rrc_delay]
    taps = (pulse_taps(sps, rolloff, rrc_delay, tau).astype(np.float64) / centre).astype(np.float32)
    lead = 301
    n = lead + lay["out_syms"] + 90
    ps = PulseShaper(sps, taps=taps, max_symbols=n + 2 * rrc_delay + 64)
    n_all = n + ps.history + 64  # the flush: history + 64 zero symbols
    d_x = torch.zeros((n_all, 2), dtype=torch.float32, device="cuda")
    d_x[:lead] = torch.from_numpy(P.qpsk(rng, lead).astype(np.complex64).view(np.float32).reshape(-1, 2)).cuda()
    fr.work_device(d_xfec.data_ptr(), len(seq), seq[-1], d_x.data_ptr() + 8 * lead, st)
    d_y = torch.zeros((n_all * sps, 2), dtype=torch.float32, device="cuda")
    ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), n_all * sps, st)
    # receive: timing recovery and matched filter, frame search, gather, coarse estimate, front end, FEC
    ns = n_all * sps
    ss = SymbolSync(sps=sps, loop_bw=0.01, damping=1.0, rolloff=rolloff, interp_method=0, max_samples=ns)
    d_sym = torch.zeros(2 * ns, dtype=torch.float32, device="cuda")
    ss.work_device(d_y.data_ptr(), ns, [ns], d_sym.data_ptr(), ns, ns, 0, 0, st)
    n_out, consumed, status = ss.finish()
    nsym = int(n_out[0])
    assert status[0] == 0 and abs(nsym - n_all) <= 12
    sync = PlSync(plsc=-1, max_symbols=max(nsym, PlSync.MIN_SYMBOLS), max_frames=64)
    d_rec = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
    sync.work_device(d_sym.data_ptr(), nsym, d_rec.data_ptr(), st)
    nf, _, state = sync.finish()
    recs = d_rec.cpu().numpy().view(PlSync.FRAME_DTYPE)[:nf]
    assert state == capi.PLSYNC_LOCKED and nf == len(seq) and recs["plsc"].tolist() == seq  # every frame found
    shifts = set((recs["sof_index"] - (lead + lay["out_offset"])).tolist())
    assert len(shifts) == 1, shifts  # one constant delay
    shift = shifts.pop()
    print(f"closed loop: {nsym} symbols from {ns} samples, SOF shift {shift} symbols (shaper delay {rrc_delay})")
    assert abs(shift - rrc_delay) <= 12  # the loop's start-up and the matched filter, moved by this stage's own delay in symbols
    locked = [f for f, r in enumerate(recs) if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == plsc]
    assert len(locked) >= nd - 1  # the tracker locks at the second header
    d_fr = torch.zeros((len(locked) * L + 90) * 2, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    sync.gather_device(d_sym.data_ptr(), d_rec.data_ptr(), nf, plsc, d_fr.data_ptr(), d_cnt.data_ptr(), st)
    torch.cuda.synchronize()
    cnt = int(d_cnt.item())
    assert cnt == len(locked)
    pc = PlCoarse(1, plsc, max_frames=64)
    d_cc = torch.zeros(cnt, dtype=torch.int32, device="cuda")
    d_f = torch.zeros(cnt, dtype=torch.float32, device="cuda")
    pc.work_device(d_fr.data_ptr(), L, cnt, 0, d_f.data_ptr(), d_cc.data_ptr(), 0, st)
    fe = PlFrontEnd(gold, plsc, max_frames=cnt)
    d_rx = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
    fe.work_device(d_fr.data_ptr(), cnt, 1, d_cc.data_ptr(), d_f.data_ptr(), d_rx.data_ptr(), st)
    torch.cuda.synchronize()
    chain = FecChain(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, group_size=4, max_frames=cnt, max_trials=25)
    chain.set_descramble(True)
    msg, ret, corr = chain.work(d_rx.cpu().numpy().view(np.complex64), np.float32(0.02))
    assert (ret >= 0).all() and (corr >= 0).all()
    data_index = [sum(1 for q in seq[:f] if q == plsc) for f in locked]  # which encoder frame each gathered frame carries
    assert np.array_equal(msg, sent[data_index])  # the encoder's input bytes
    for o in (chain, fe, pc, sync, ss, ps, fr, enc):
        o.close()
