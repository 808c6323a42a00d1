"""Resampler on the device (dvbs2_resamp_*) against the float32 model (a) of tests/resamp_model.py: every output sample BIT FOR BIT
(uint32 compare) into sentinel-filled buffers whose pads and gaps must stay untouched, with zeros of both signs and denormals planted
in the input; the device's positions against the model's Python integers after every call; then two closed loops through the receive
stages of this library: a sampling-clock offset that symsync has to track, and the fractional-sps transmitter with its way back."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import pulse_model as PM
import resamp_model as RM
from dvbs2rx_amd import PulseShaper, Resampler, SymbolSync, capi, plframer_layout, pulse_taps, resamp_geometry, resamp_max_out, resamp_step
from fec_testlib import PAD, SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu

K = capi.RESAMP_TILE   # the kernel's tile in output samples
ODD_STEP = (1 << 32) + 0x9E3779B1  # a raw step that uses all 32 fraction bits (rate about 0.62)


class Model:
    """model (a) of one stream with its history and position"""

    def __init__(self, taps, nfilts, step, acc=0):
        self.taps, self.nfilts, self.step, self.acc, self.hist = taps, nfilts, step, acc, None

    def work(self, x):
        y, self.hist, self.acc = RM.resample32(self.taps, self.nfilts, x, self.step, self.acc, self.hist)
        return y


def run_on_device(rs, xs, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the streams xs (complex64 vectors of one length n) through fec_testlib.run_strided: stream s lies at
    in_shift + s * in_stride complex elements of the input buffer and writes at out_shift + s * out_stride of a sentinel buffer, where
    nothing but the n_out[s] samples produce() gave before the call may be written. Returns (one uint32 (n_out[s], 2) array per stream,
    n_out) after checking that the reported counts are those produce() gave."""
    ns, n = len(xs), xs[0].size
    said = rs.produce(n, ns)
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(int(said.max()), 1) if out_stride is None else out_stride
    outs, n_out = T.run_strided(lambda a, o: rs.work_device(a, in_stride, n, ns, o, out_stride, stream()), xs, [int(k) for k in said],
                                in_stride, out_stride, in_shift, out_shift)
    assert np.array_equal(n_out, said), (n_out, said)
    return outs, n_out


def same(got, want, what):
    T.same_bits(got, RM.bits(want), what)


def state_is(rs, models, what):
    """the device's positions against the model's (Python integers), and the host mirror through produce()"""
    acc = rs.state()
    assert [int(a) for a in acc[:len(models)]] == [m.acc for m in models], what
    for n_in in (0, 1, 97):
        assert rs.produce(n_in, len(models)).tolist() == [RM.advance(m.acc, m.step, n_in)[0] for m in models], what


@functools.lru_cache(maxsize=None)
def data(seed, n):
    x = PM.planted(np.random.default_rng(seed), n)
    x.setflags(write=False)
    return x


def call_for(step, target):
    """(n_in, frac): the shortest call and an initial position below 2^32 that give exactly `target` outputs"""
    n_in = 1
    while RM.max_out(step, n_in) < target:
        n_in += 1
    frac = max(0, (n_in << 32) - target * step)
    assert frac < 1 << 32 and RM.advance(frac, step, n_in)[0] == target
    return n_in, frac


def check_calls(rs, taps, nfilts, step, calls, what):
    """each (n_in, frac) from a reset handle, then a second call of 40 samples that continues from its history and position"""
    for n_in, frac in calls:
        rs.reset()
        if frac:
            rs.reset_phase([frac])
        m = Model(taps, nfilts, step, frac)
        x, more = data(nfilts * 1000 + n_in % 997, max(n_in, 1))[:n_in], data(7, 40)
        same(run_on_device(rs, [x])[0][0], m.work(x), f"{what}: {n_in} samples from {frac:#x}")
        state_is(rs, [m], f"{what}: {n_in} samples from {frac:#x}")
        same(run_on_device(rs, [more])[0][0], m.work(more), f"{what}: 40 samples behind {n_in}")
        state_is(rs, [m], f"{what}: 40 samples behind {n_in}")


# ------------------------------------------------------------------ 1. rates and shapes
RATES = {"1": 1 << 32, "1+1e-4": RM.step_of(1 + 1e-4), "2.5": RM.step_of(2.5), "0.8": RM.step_of(0.8), "0.5": 1 << 33, "64": 1 << 26,
         "odd": ODD_STEP}


@pytest.mark.parametrize("rate", list(RATES))
def test_designed_prototype_at_every_rate(rate):
    """nfilts 32, the transmit prototype with D = 5: L = 11. Input lengths 1, L - 2, L - 1, L, and the lengths and initial positions
    that put n_out at K - 1, K, K + 1 and 3 K + 7."""
    step, nfilts = RATES[rate], 32
    taps = pulse_taps(nfilts, 0.2, 5, 0.0, nfilts)
    L, H, delay_num = resamp_geometry(nfilts, taps.size)
    assert (L, H, delay_num) == (11, 10, 160)
    calls = [(n, 0) for n in (1, L - 2, L - 1, L)] + [call_for(step, t) for t in (K - 1, K, K + 1, 3 * K + 7)]
    rs = Resampler(nfilts, taps, 1.0, max_samples=max(97, max(n for n, _ in calls)))  # (97: what state_is asks produce() about)
    assert (rs.nfilts, rs.ntaps, rs.terms, rs.history, rs.delay_num, rs.step) == (nfilts, taps.size, L, H, delay_num, 1 << 32)
    rs.set_step(step)
    assert rs.step == step
    check_calls(rs, taps, nfilts, step, calls, f"rate {rate}")
    rs.close()


def test_branch_changes_inside_a_wavefront():
    """1 + 1e-4: the fraction falls by about 429453 per output, a branch (2^27) lasts about 312 outputs. From 20 outputs above a
    branch boundary, 1500 samples cross the first boundary at lane 21 of the first wavefront and four more further on."""
    nfilts, step = 32, RM.step_of(1 + 1e-4)
    taps = pulse_taps(nfilts, 0.2, 5, 0.0, nfilts)
    frac = (3 << 27) + 20 * ((1 << 32) - step) + 7
    j = RM.split([frac + m * step for m in range(64)], 5)[1]
    assert j[0] == 3 and j[63] == 2 and 0 < np.count_nonzero(j == 3) < 64
    rs = Resampler(nfilts, taps, 1 + 1e-4, max_samples=1500)
    assert rs.step == step == resamp_step(1 + 1e-4)
    check_calls(rs, taps, nfilts, step, [(1500, frac)], "1 + 1e-4 across branch boundaries")
    rs.close()


@pytest.mark.parametrize("nfilts,ntaps", [(2, 1), (2, 256), (2, 7), (256, 1), (256, 8192), (256, 1000)])
def test_callers_taps_with_ragged_branches(nfilts, ntaps):
    """ntaps = 1: every branch but 0 has no tap (its samples are +0.0) and there is no history; (2, 256) the cap of 128 terms and 127
    samples of history; (256, 8192) the cap of 8192 taps, the largest bank in LDS; (2, 7) and (256, 1000) branches with L and L - 1
    terms."""
    rng = np.random.default_rng(ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    L, H, _ = resamp_geometry(nfilts, ntaps)
    rs = Resampler(nfilts, taps, 1.0, max_samples=2 * K)
    assert (rs.terms, rs.history) == (L, H) == RM.geometry(nfilts, ntaps)[:2]
    for step in (RATES["2.5"], ODD_STEP):
        rs.set_step(step)
        calls = [(1, 0), (max(H, 1) + 1, 0x80000001), call_for(step, K + 1)]
        check_calls(rs, taps, nfilts, step, calls, f"nfilts {nfilts} ntaps {ntaps} step {step:#x}")
    if ntaps == 1:
        rs.reset()
        rs.set_step(RATES["2.5"])
        got = run_on_device(rs, [data(3, 100)])[0][0]
        j = RM.split([m * RATES["2.5"] for m in range(got.shape[0])], nfilts.bit_length() - 1)[1]
        assert (got[j != 0] == 0).all() and (j != 0).any()  # +0.0, not -0.0
    rs.close()


# ------------------------------------------------------------------ 2. streaming
@pytest.mark.parametrize("rate", ["2.5", "0.8", "1+1e-4"])
def test_pieces_give_the_bits_of_one_call(rate):
    step, nfilts = RATES[rate], 32
    taps = pulse_taps(nfilts, 0.2, 5, 0.0, nfilts)
    n = 2 * K + 61
    rs = Resampler(nfilts, taps, 1.0, max_samples=n)
    rs.set_step(step)
    L = rs.terms
    x = data(40, n)
    m = Model(taps, nfilts, step)
    whole = run_on_device(rs, [x])[0][0]
    same(whole, m.work(x), "one call")
    state_is(rs, [m], "one call")
    rs.reset()
    m = Model(taps, nfilts, step)
    cuts = [1, 0, L - 2, 2, K + 3]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    parts, pos = [], 0
    for c in cuts:
        parts.append(run_on_device(rs, [x[pos:pos + c]])[0][0])
        m.work(x[pos:pos + c])
        state_is(rs, [m], f"after {pos + c} samples")
        pos += c
    assert np.array_equal(np.concatenate(parts), whole), cuts
    rs.reset()  # the first-call result again
    assert np.array_equal(run_on_device(rs, [x])[0][0], whole)
    rs.close()


def test_set_rate_between_calls():
    """a drifting clock is a sequence of calls: the new step holds from the next call, the position is carried over"""
    nfilts = 32
    taps = pulse_taps(nfilts, 0.35, 8, 0.0, nfilts)
    rs = Resampler(nfilts, taps, 1 + 1e-4, max_samples=700)
    m = Model(taps, nfilts, RM.step_of(1 + 1e-4))
    for i, (rate, n) in enumerate(((None, 700), (1 - 1e-4, 300), (2.5, 5), (0.5, 600), (64.0, 9), (1.0, 200))):
        if rate is not None:
            rs.set_rate(rate)
            m.step = RM.step_of(rate)
            assert rs.step == m.step
        x = data(50 + i, n)
        same(run_on_device(rs, [x])[0][0], m.work(x), f"call {i} at rate {rate}")
        state_is(rs, [m], f"call {i} at rate {rate}")
    rs.close()


# ------------------------------------------------------------------ 3. batches
def test_streams_keep_their_own_history_and_position():
    """3 streams with strides larger than the data over four calls, one of them on two of the streams only; distinct initial positions,
    so that the n_out[s] of one call differ."""
    nfilts, step = 32, RATES["0.8"]
    taps = pulse_taps(nfilts, 0.2, 5, 0.0, nfilts)
    rs = Resampler(nfilts, taps, 0.8, max_streams=3, max_samples=K + 9)
    frac = [0, 0xFFFFFFFF, 0x40000000]
    rs.reset_phase(frac)
    models = [Model(taps, nfilts, step, f) for f in frac]
    state_is(rs, models, "after reset_phase")
    n1, n2 = K + 9, 7  # the second call is shorter than the history: old history and input both enter the new one
    first = [data(20 + s, n1) for s in range(3)]
    second = [data(30 + s, n2) for s in range(3)]
    differed = False
    for what, xs, in_stride, pad_out in (("first", first, n1 + 3, 5), ("second", second, n2 + 1, 6), ("third", second[:2], n2, 0),
                                         ("fourth", first, n1, 1)):
        most = int(rs.produce(xs[0].size, len(xs)).max())
        got, n_out = run_on_device(rs, xs, in_stride=in_stride, out_stride=most + pad_out)
        differed |= len(set(n_out.tolist())) > 1
        for s in range(len(xs)):
            same(got[s], models[s].work(xs[s]), f"stream {s}, {what} call")
        state_is(rs, models, f"{what} call")
    assert differed
    rs.close()


# ------------------------------------------------------------------ 4. alignment
@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_alignment(in_shift, out_shift):
    """Buffers displaced by one complex element are 8-byte but not 16-byte aligned: the same bits."""
    nfilts, step = 32, RATES["2.5"]
    taps = pulse_taps(nfilts, 0.2, 5, 0.0, nfilts)
    rs = Resampler(nfilts, taps, 2.5, max_samples=K // 2 + 7)
    x = data(60, K // 2 + 7)
    same(run_on_device(rs, [x], in_shift=in_shift, out_shift=out_shift)[0][0], Model(taps, nfilts, step).work(x), f"shifts {in_shift} {out_shift}")
    rs.close()


# ------------------------------------------------------------------ 5. the host entry
def test_host_entry_equals_the_device_entry():
    nfilts = 16
    taps = pulse_taps(40, 0.2, 5, 0.0, 16.0)
    a, b = Resampler(nfilts, taps, 0.8, max_samples=K + 30), Resampler(nfilts, taps, 0.8, max_samples=K + 30)
    m = Model(taps, nfilts, RATES["0.8"])
    for n in (K + 30, 3, 0, 1, 50):
        x = data(70 + n, max(n, 1))[:n]
        got = a.work(x)
        want = m.work(x)
        assert got.dtype == np.complex64
        same(RM.bits(got).reshape(-1, 2), want, f"host entry, {n} samples")
        if n:
            assert np.array_equal(run_on_device(b, [x])[0][0], RM.bits(got).reshape(-1, 2))
        assert np.array_equal(a.state(), b.state()) and int(a.state()[0]) == m.acc
    a.close()
    b.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_everything_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    good_taps = np.ones(21, np.float32)
    # creation (every argument refusal without a device: tests/test_resamp_model.py)
    refused(capi.EINVAL, "nfilts must be a power of two in 2..256", lib.dvbs2_resamp_create, C.byref(h), 3, good_taps.ctypes.data, 21, 1.0, 1, 16, 0)
    refused(capi.EINVAL, "rate must lie in [0.5, 64]", lib.dvbs2_resamp_create, C.byref(h), 2, good_taps.ctypes.data, 21, 0.25, 1, 16, 0)
    refused(capi.EINVAL, "null handle pointer", lib.dvbs2_resamp_create, None, 2, good_taps.ctypes.data, 21, 1.0, 1, 16, 0)
    assert not h
    assert lib.dvbs2_resamp_create(C.byref(h), 2, good_taps.ctypes.data, 21, 1.0, 1, 16, 99) < 0 and not h  # no such device

    nfilts, step, n = 32, RATES["2.5"], 100
    taps = pulse_taps(nfilts, 0.2, 5, 0.0, nfilts)
    rs = Resampler(nfilts, taps, 2.5, max_streams=2, max_samples=n)
    rs.reset_phase([0, 0x12345678])
    models = [Model(taps, nfilts, step, 0), Model(taps, nfilts, step, 0x12345678)]
    first, second = [data(80 + s, n) for s in range(2)], [data(90 + s, n) for s in range(2)]
    got, _ = run_on_device(rs, first)
    for s in range(2):
        same(got[s], models[s].work(first[s]), f"stream {s} before the refusals")
    most = int(rs.produce(n, 2).max())
    assert 250 <= most <= resamp_max_out(step, n) == 251  # (the step is 2^32 / 2.5 rounded down: a hair above 2.5)
    d_in = torch.from_numpy(np.concatenate(second).view(np.float32)).cuda()
    d_out = sentinel(2 * (2 * most + PAD))
    st = stream()
    a, o = d_in.data_ptr(), d_out.data_ptr()
    counts = np.full(2, -7, np.int64)
    c = counts.ctypes.data
    entry = lib.dvbs2_resamp_process_device
    refused(capi.ESIZE, "n_in exceeds max_samples", entry, rs._h, a, n, n + 1, 1, o, most, c, st)
    refused(capi.ESIZE, "n_streams exceeds max_streams", entry, rs._h, a, n, n, 3, o, most, c, st)
    refused(capi.EINVAL, "in_stride is below n_in", entry, rs._h, a, n - 1, n, 2, o, most, c, st)
    refused(capi.EINVAL, "out_stride is below the call's largest n_out", entry, rs._h, a, n, n, 2, o, most - 1, c, st)
    refused(capi.EINVAL, "out_stride is below the call's largest n_out", entry, rs._h, a, n, n, 1, o, most - 1, c, st)
    refused(capi.EINVAL, "in is null", entry, rs._h, None, n, n, 2, o, most, c, st)
    refused(capi.EINVAL, "out is null", entry, rs._h, a, n, n, 2, None, most, c, st)
    refused(capi.EINVAL, "n_in is negative", entry, rs._h, a, n, -1, 2, o, most, c, st)
    refused(capi.EINVAL, "n_streams is negative", entry, rs._h, a, n, n, -1, o, most, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, rs._h, a + 4, n, n, 2, o, most, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, rs._h, a, n, n, 2, o + 4, most, c, st)
    assert (counts == -7).all()
    refused(capi.EINVAL, "step must lie in [2^26, 2^33]", lib.dvbs2_resamp_set_step, rs._h, (1 << 26) - 1)
    refused(capi.EINVAL, "step must lie in [2^26, 2^33]", lib.dvbs2_resamp_set_step, rs._h, (1 << 33) + 1)
    refused(capi.EINVAL, "rate must lie in [0.5, 64]", lib.dvbs2_resamp_set_rate, rs._h, 0.4)
    refused(capi.EINVAL, "rate must lie in [0.5, 64]", lib.dvbs2_resamp_set_rate, rs._h, float("nan"))
    assert rs.step == step
    refused(capi.ESIZE, "n_in exceeds max_samples", lib.dvbs2_resamp_produce, rs._h, n + 1, 1, c)
    refused(capi.ESIZE, "n_streams exceeds max_streams", lib.dvbs2_resamp_produce, rs._h, n, 3, c)
    refused(capi.EINVAL, "n_in is negative", lib.dvbs2_resamp_produce, rs._h, -1, 1, c)
    refused(capi.EINVAL, "n_streams is negative", lib.dvbs2_resamp_produce, rs._h, n, -1, c)
    refused(capi.EINVAL, "n_out is null", lib.dvbs2_resamp_produce, rs._h, n, 1, None)
    refused(capi.EINVAL, "acc is null", lib.dvbs2_resamp_state, rs._h, None)
    assert (counts == -7).all()
    assert entry(rs._h, None, 0, 0, 2, None, 0, c, st) == capi.OK  # n_in == 0: a successful call that does nothing and reports zeros
    assert counts.tolist() == [0, 0]
    assert entry(rs._h, a, 0, n, 0, o, 0, None, st) == capi.OK
    state_is(rs, models, "behind the refusals")
    assert entry(rs._h, a, 0, n, 1, o, most, None, st) == capi.OK  # one stream: in_stride does not matter; no counts wanted
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    want0 = models[0].work(second[0])
    same(out[:want0.size], want0, "the one-stream call behind the refusals")
    assert (out[want0.size:] == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = second[0].copy(), np.zeros(most, np.complex64)
    n_out = C.c_int64(-7)
    host = lib.dvbs2_resamp_process
    refused(capi.ESIZE, "n_in exceeds max_samples", host, rs._h, host_in.ctypes.data, n + 1, host_out.ctypes.data, most, C.byref(n_out))
    refused(capi.EINVAL, "n_in is negative", host, rs._h, host_in.ctypes.data, -1, host_out.ctypes.data, most, C.byref(n_out))
    refused(capi.EINVAL, "in is null", host, rs._h, None, n, host_out.ctypes.data, most, C.byref(n_out))
    refused(capi.EINVAL, "out is null", host, rs._h, host_in.ctypes.data, n, None, most, C.byref(n_out))
    refused(capi.EINVAL, "out_cap is negative", host, rs._h, host_in.ctypes.data, n, host_out.ctypes.data, -1, C.byref(n_out))
    refused(capi.EINVAL, "out_cap is below n_out", host, rs._h, host_in.ctypes.data, n, host_out.ctypes.data,
            int(rs.produce(n)[0]) - 1, C.byref(n_out))
    assert lib.dvbs2_resamp_process(rs._h, None, 0, None, 0, None) == capi.OK
    assert (host_out == 0).all() and n_out.value == 0
    # no refusal touched a history, a position or the mirror: both streams go on from where the good calls left them
    state_is(rs, models, "behind the host entry's refusals")
    got, _ = run_on_device(rs, first)
    for s in range(2):
        same(got[s], models[s].work(first[s]), f"stream {s} behind the refusals")
    state_is(rs, models, "the last call")
    rs.close()


# ------------------------------------------------------------------ 7. and 8. closed loops through the receiver, noise-free
SEQ, PLSC, ND, LEAD = L.SEQ6, L.PLSC, 6, 301


@functools.lru_cache(maxsize=None)
def transmitted():
    """The transmit side up to the PL framer (loopback.transmit_symbols): six short QPSK 1/4 frames and two dummy frames behind LEAD
    random symbols, 256 zero symbols behind them: more than the histories of all stages behind. Returns (the encoder's input, the
    symbols on the device, their number with the flush)."""
    sent, d_x, _, n_all, _ = L.transmit_symbols(SEQ, ND, L.GOLD, LEAD, seed=2026, flush=256)
    return sent, d_x, n_all


def receive(d_y, ns, n_syms, interp_method, sent, what):
    """d_y: ns samples at 2 per symbol on the device. Timing recovery, frame search and the decode tail of tests/loopback.py. Requires
    every frame at ONE constant symbol shift from LEAD + out_offset[f] and the encoder's input out of the chain; returns (the shift, the
    number of symbols)."""
    lay = plframer_layout(SEQ)
    rx = L.timing_and_frames(d_y, ns, 2, 0.2, interp_method, n_syms, tol=24)
    recs, nf, nsym = rx.recs, rx.nf, rx.nsym
    print(f"{what}: {nsym} symbols from {ns} samples ({n_syms} sent), status 0, loop {rx.loop}")  # (a status other than 0 does not come back from timing_and_frames)
    shifts = (recs["sof_index"] - (LEAD + lay["out_offset"][:nf])).tolist() if nf <= len(SEQ) else []
    print(f"{what}: {nf} frames, PLSCs {recs['plsc'].tolist()}, SOF shifts {shifts}")
    assert rx.state == capi.PLSYNC_LOCKED and nf == len(SEQ) and recs["plsc"].tolist() == SEQ, what  # every frame found
    assert len(set(shifts)) == 1, (what, shifts)  # one constant delay: no cycle slip
    got = L.decode_frames(rx, PLSC, L.GOLD, 0.02)
    assert len(got.locked) >= ND - 1, what  # the tracker locks at the second header
    assert np.array_equal(got.msg, sent[got.data_index]), what  # the encoder's input bytes
    rx.sync.close()
    return shifts[0], nsym


@functools.lru_cache(maxsize=None)
def shaped_at_two():
    """transmitted() through the shaper at sps 2, tau = 0, scaled for unit symbol amplitude behind the receiver's matched filter
    (loopback.unit_amplitude_taps)"""
    import torch
    sent, d_x, n_all = transmitted()
    sps = 2
    ps = PulseShaper(sps, taps=L.unit_amplitude_taps(sps, 0.2, 5), max_symbols=n_all)
    d_y = torch.zeros((n_all * sps, 2), dtype=torch.float32, device="cuda")
    ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), n_all * sps, stream())
    torch.cuda.synchronize()
    ps.close()
    return d_y


CLOCK_PPM = 100  # the largest of 100, 50, 20 that the loop holds (notes/resampler.md has all three outcomes)


@pytest.mark.parametrize("ppm", [0, CLOCK_PPM, -CLOCK_PPM])
def test_closed_loop_with_a_sampling_clock_offset(ppm):
    """A: the shaper's samples at 2 per symbol through this stage at rate 1 + ppm 1e-6 (prototype dvbs2_pulse_taps(32, 0.35, 8, 0, 32):
    flat below 0.325 cycles per sample, the signal ends at 0.3), then symsync with the polyphase matched filter. Over the 114 thousand
    samples 100 ppm are 11 samples of drift: the loop has to follow them without a cycle slip. ppm = 0 is the control: rate exactly 1."""
    import torch
    sent, _, n_all = transmitted()
    d_y = shaped_at_two()
    ns = 2 * n_all
    nfilts = 32
    rs = Resampler(nfilts, pulse_taps(nfilts, 0.35, 8, 0.0, nfilts), 1 + ppm * 1e-6, max_samples=ns)
    assert (rs.step == 1 << 32) == (ppm == 0)
    n_out = int(rs.produce(ns)[0])
    assert abs(n_out - ns * (1 + ppm * 1e-6)) <= 1
    d_z = torch.zeros((n_out, 2), dtype=torch.float32, device="cuda")
    assert rs.work_device(d_y.data_ptr(), ns, ns, 1, d_z.data_ptr(), n_out, stream())[0] == n_out
    shift, nsym = receive(d_z, n_out, n_all, SymbolSync.POLYPHASE, sent, f"clock offset {ppm} ppm")
    # the shaper's delay (5 symbols), this stage's (8 input samples: 4 symbols), the matched filter and the loop's start-up
    assert abs(shift - 9) <= 12
    rs.close()


def test_closed_loop_through_the_fractional_sps_transmitter():
    """B: the PL framer's symbols straight into this stage at rate 2.5 (32 branches of dvbs2_pulse_taps(32, 0.2, 5, 0, 32): the
    fractional branch of the reference's transmitter), a second handle at rate 0.8 whose prototype dvbs2_pulse_taps(40, 0.2, 5, 0, 16) is
    the matched filter at 16 taps per input sample (40 per symbol), then symsync with the cubic interpolator, so that nothing filters
    twice. The transmit taps are scaled for unit symbol amplitude: by the peak of the response of both stages to one unit symbol, from
    model (b)."""
    import torch
    sent, d_x, n_all = transmitted()
    tx = pulse_taps(32, 0.2, 5, 0.0, 32.0)
    rx = pulse_taps(40, 0.2, 5, 0.0, 16.0)
    impulse = np.zeros(48, np.complex64)
    impulse[0] = 1.0
    mid = RM.resample64(tx, 32, impulse, RATES["2.5"])[0].astype(np.complex64)
    peak = np.abs(RM.resample64(rx, 16, mid, RATES["0.8"])[0]).max()
    assert 0.5 < peak < 2.0
    tx = (tx.astype(np.float64) / peak).astype(np.float32)
    up = Resampler(32, tx, 2.5, max_samples=n_all)
    n_mid = int(up.produce(n_all)[0])
    assert abs(n_mid - 2.5 * n_all) <= 1
    d_mid = torch.zeros((n_mid, 2), dtype=torch.float32, device="cuda")
    up.work_device(d_x.data_ptr(), n_all, n_all, 1, d_mid.data_ptr(), n_mid, stream())
    down = Resampler(16, rx, 0.8, max_samples=n_mid)
    ns = int(down.produce(n_mid)[0])
    assert abs(ns - 2 * n_all) <= 1
    d_y = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
    down.work_device(d_mid.data_ptr(), n_mid, n_mid, 1, d_y.data_ptr(), ns, stream())
    shift, nsym = receive(d_y, ns, n_all, SymbolSync.CUBIC, sent, "fractional sps 2.5")
    assert abs(shift - 10) <= 12  # 5 symbols in each of the two stages, and the loop's start-up
    up.close()
    down.close()
