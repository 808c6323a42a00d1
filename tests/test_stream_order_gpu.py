"""Every stage's stream contract on a BUSY non-blocking stream (include/dvbs2_fec_hip.h: "asynchronous on `stream`", "no host
synchronisation", "waits for the device", "waits for the last call", "takes effect from the next call").

The rest of the suite calls the stages on the null stream, or on an idle side stream with a synchronisation behind every call: there
every synchronous hipMemcpy / hipMemset inside a stage is ordered against the stage's kernels for free. Here a bounded spin
(fec_testlib.hold) is enqueued on a non-blocking stream first, so that everything a test enqueues behind it is still PENDING while the
host goes on, and
  A. a sequence of calls enqueued back to back with no host synchronisation equals the same sequence serialized, and
  B. an entry that promises to wait, called while work of the handle is pending, gives what it gives in the serialized order.
One table of rows (ROWS): make() the handle(s), prep() every device buffer, then a list of calls -- ("call", f) enqueues on the stream,
("wait", f) is an entry whose header comment says it waits -- and collect() every output, reported count and state getter as bytes.
The EXPECTED value of a row is the same calls on a fresh handle on the null stream with a synchronise behind each call, and that
serialized pass is itself tied to the stage's model (tests/*_model.py, the CPU oracle) by the row's model(): it is never just the code
under test on another stream. A held pass asserts that the stream was still pending behind its last enqueue (A) or just before the
waiting entry (B): a stream that had drained is a failure -- the hold was too short or an entry synchronised the host.
Hold lengths are measured (fec_testlib.hold_for): 20 times the host time of the enqueues of the serialized pass, at least 20 ms.
Every value a test changes behind a call's back (a selection, an n_in array) is another LEGAL value: a lost race gives wrong bits,
never a wild index. notes/stream_order.md has the calibration, the host times and what the two probes of the runtime saw."""
import ctypes as C
import functools
import time
from types import SimpleNamespace as NS

import numpy as np
import pytest

import agc_model as AM
import awgn_model as WM
import bbframer_model as BM
import ddc_model as DM
import demap_table_model as DT
import fec_testlib as T
import iqconv_model as IQ
import pfbch_model as CM
import pfbsyn_model as YM
import plcoarse_model as K
import plframe_model as M
import plframer_model as F
import plsync_model as P
import pulse_model as PM
import resamp_model as RM
import spectrum_model as SM
import symsync_model as S
from dvbs2rx_amd import (Agc, Awgn, BbDeheader, BbFramer, BchDecoder, Ddc, Demapper, FecEncoder, IqConverter, PfbChannelizer,
                         PfbSynthesizer, PlCoarse, PlFramer, PlFrontEnd, PlPayload, PlSync, PulseShaper, Resampler, Rotator, Spectrum,
                         SymbolSync, capi, get_fec_info, pls_parse, pulse_taps, spectrum_twiddles, spectrum_window, symsync_taps)
from dvbs2rx_amd.capi import lib

pytestmark = pytest.mark.gpu

SHORT, QPSK = capi.FECFRAME_SHORT, capi.MOD_QPSK
TABLE = "S2_TABLE_C1"  # QPSK 1/4 short
FEC = get_fec_info(capi.STANDARD_DVBS2, SHORT, "C1_4")  # host only


def cplx(key, *shape):
    rng = np.random.default_rng([113, key])
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


def dev(a):
    import torch
    a = np.array(a, order="C")  # a copy: the shared inputs are read-only
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def zeros(n, dtype="float32"):
    import torch
    return torch.zeros(int(n), dtype=getattr(torch, dtype), device="cuda")


def host(t):
    return t.cpu().numpy()


def p(t, elements=0, size=8):
    """the address `elements` elements of `size` bytes into a device tensor"""
    return t.data_ptr() + size * int(elements)


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def exact(**want):
    """model(): these outputs of the serialized pass are the model's, bit for bit"""
    def check(got):
        for k, w in want.items():
            assert raw(got[k]) == raw(w), f"{k}: the serialized pass is not the model"
    return check


def spans(cuts):
    a = np.concatenate([[0], np.cumsum(cuts)])
    return [(int(u), int(v - u)) for u, v in zip(a[:-1], a[1:])]


class Row:
    """name; handle: the capi handle types the row exercises; make() -> o; prep(o) -> c (every device buffer, nothing allocated
    later); calls: [(kind, f(o, c, s))] with kind "call" or "wait" and s the stream as an integer (0: the null stream);
    collect(o, c) -> {name: array}; model(got): asserts the serialized pass against the model; check(got): what must hold in every
    pass (e.g. the bits behind a reset are those in front of it)."""

    def __init__(self, name, handle, make, prep, calls, collect, model=None, check=None):
        self.name, self.handle, self.make, self.prep, self.collect, self.model, self.check = name, handle, make, prep, collect, model, check
        self.calls = [c if isinstance(c, tuple) else ("call", c) for c in calls]

    @property
    def waits(self):
        return any(kind == "wait" for kind, _ in self.calls)


def close(o):
    for h in (o if isinstance(o, (tuple, list)) else (o,)):
        h.close()


def run_serialized(row):
    """(outputs, host seconds of the enqueues): every call on the null stream, a synchronise behind each"""
    import torch
    o = row.make()
    c = row.prep(o)
    torch.cuda.synchronize()
    spent = 0.0
    for _, f in row.calls:
        t0 = time.perf_counter()
        f(o, c, 0)
        spent += time.perf_counter() - t0
        torch.cuda.synchronize()
    got = row.collect(o, c)
    close(o)
    return got, spent


@functools.lru_cache(None)
def reference(name):
    """The serialized pass of a row, twice: the first loads every code object and is the expected value -- checked against the
    model --, the second must repeat it and gives the host time of the enqueues on a warm handle."""
    row = get_row(name)
    want, _ = run_serialized(row)
    if row.model is not None:
        row.model(want)
    if row.check is not None:
        row.check(want)
    again, spent = run_serialized(row)
    same(again, want, f"{name}: the serialized pass, repeated")
    return want, spent * 1e3


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.frombuffer(raw(got[k]), np.uint8), np.frombuffer(raw(want[k]), np.uint8)
        assert g.size == w.size, (what, k, g.size, w.size)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {k}: {bad.size} of {w.size} bytes differ, the first at byte {bad[0]}")


def run_held(row, side, hold_ms):
    """the row's calls behind a hold on `side`; asserts pending behind the last enqueue, or just before each waiting entry"""
    import torch
    o = row.make()
    c = row.prep(o)
    torch.cuda.synchronize()
    T.hold(side, hold_ms)
    for i, (kind, f) in enumerate(row.calls):
        if kind == "wait":
            assert T.pending(side), f"{row.name}: the stream had drained before the waiting entry (call {i}): hold {hold_ms:.0f} ms too short, or an entry synchronised"
        f(o, c, side.cuda_stream)
    still = T.pending(side)
    side.synchronize()
    assert still or row.waits, f"{row.name}: the stream had drained behind the last enqueue: hold {hold_ms:.0f} ms too short, or an entry synchronised the host"
    torch.cuda.synchronize()
    got = row.collect(o, c)
    close(o)
    return got


# ================================================================== the rows
ROWS = {}  # name -> how to build the row; built when first asked for (get_row), so that collecting this file needs no device


def row(name, build, *args, **kwargs):
    assert name not in ROWS
    ROWS[name] = functools.partial(build, name, *args, **kwargs)


@functools.lru_cache(None)
def get_row(name):
    return ROWS[name]()


# ------------------------------------------------------------------ agc
def agc_row(name, rate=0.05, after_first=None, n_rows=2):
    """cuts below, at and above the tile of 64 samples; after_first: a waiting entry between the first call and the others"""
    cuts = [Agc.TILE - 1, Agc.TILE, Agc.TILE + 9]
    n = sum(cuts)
    x = cplx(1, n_rows, n)

    def prep(o):
        return NS(x=dev(x), y=zeros(2 * n_rows * n), g=zeros(n_rows * n), said=[])

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, a), n, k, n_rows, p(c.y, a), n, p(c.g, a, 4), n, s)

    calls = [call(a, k) for a, k in spans(cuts)]
    m = AM.AgcModel(rate, 1.0, 1.0, 65536.0, n_rows)
    if after_first is None:
        out, gains = m.work(x)
    else:
        kind, f, on_model = after_first
        calls.insert(1, (kind, f))
        o0, g0 = m.work(x[:, :cuts[0]])
        said = on_model(m)
        o1, g1 = m.work(x[:, cuts[0]:])
        out, gains = np.concatenate([o0, o1], axis=1), np.concatenate([g0, g1], axis=1)
    want = dict(out=out, gain=gains, state=m.g.copy())
    if after_first is not None and said is not None:
        want["said"] = said
    return Row(name, "agc", lambda: Agc(rate, 1.0, 1.0, 65536.0, max_streams=n_rows, max_samples=2 * Agc.TILE), prep, calls,
               lambda o, c: dict(out=host(c.y), gain=host(c.g), state=o.state(), said=np.array(c.said, np.float32)), exact(**want))


def _agc_state(o, c, s):
    c.said.extend(o.state().tolist())


row("agc", agc_row)
row("agc-other", agc_row, rate=0.01)
row("agc-reset", agc_row, after_first=("wait", lambda o, c, s: o.reset(), lambda m: m.reset()))
row("agc-set_gain", agc_row, after_first=("wait", lambda o, c, s: o.set_gain(1, 0.25), lambda m: m.set_gain(1, 0.25)))
row("agc-state", agc_row, after_first=("wait", _agc_state, lambda m: m.g.copy()))


# ------------------------------------------------------------------ awgn
def awgn_row(name):
    cuts = [Awgn.TILE - 1, Awgn.TILE, Awgn.TILE + 1]
    n, first = sum(cuts), 10
    x = cplx(2, 2, n)

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, a), n, k, 2, p(c.y, a), n, first_stream=3, first_index=first + a, stream=s)

    want = WM.rows(5, 3, first, n, 2, np.float32(0.75), x.view(np.float32).reshape(2, n, 2)).astype(np.float32)
    return Row(name, "awgn", lambda: Awgn(seed=5, sigma=0.75, max_streams=2, max_samples=Awgn.TILE + 1),
               lambda o: NS(x=dev(x), y=zeros(4 * n)), [call(a, k) for a, k in spans(cuts)], lambda o, c: dict(out=host(c.y)), exact(out=want))


row("awgn", awgn_row)


# ------------------------------------------------------------------ iqconv: three unpack calls, then one pack call over what they wrote
def iqconv_row(name):
    cuts = [IqConverter.TILE - 1, IqConverter.TILE, IqConverter.TILE + 1]
    n = sum(cuts)
    codes = np.random.default_rng(3).integers(0, 256, (2, n, 2)).astype(np.uint8)

    def prep(o):
        return NS(codes=dev(codes), y=zeros(4 * n), back=zeros(4 * n, "uint8"), stats=zeros(2 * 2 * 3, "int64"))

    def unpack(a, k):
        return lambda o, c, s: o.unpack_device(p(c.codes, a, 2), n, k, 2, p(c.y, a), n, p(c.stats), s)

    calls = [unpack(a, k) for a, k in spans(cuts)]
    calls.append(lambda o, c, s: o.pack_device(p(c.y), n, n, 2, p(c.back), n, p(c.stats, 6), s))
    y, st_u = IQ.unpack_rows(IQ.U8, 1.0, codes)
    back, st_p = IQ.pack_rows(IQ.U8, 1.0, y)
    return Row(name, "iqconv", lambda: IqConverter("u8", 1.0, max_streams=2, max_samples=n), prep, calls,
               lambda o, c: dict(out=host(c.y), back=host(c.back), stats=host(c.stats)),
               exact(out=y, back=back, stats=np.array([st_u, st_p], np.uint64)))


row("iqconv", iqconv_row)


# ------------------------------------------------------------------ pulse
def pulse_row(name, sps=2, reset_after_first=False):
    taps = pulse_taps(sps, 0.2, 5)
    H = PM.history_of(taps.size, sps)
    cuts = [H - 1, H, PulseShaper.TILE + 1]
    n = sum(cuts)
    x = cplx(4, 2, n)

    def call(a, k, b=None):
        b = a if b is None else b
        return lambda o, c, s: o.work_device(p(c.x, a), n, k, 2, p(c.y, sps * b), sps * 2 * n, s)

    sp = spans(cuts)
    if reset_after_first:  # the first cut, reset, the first cut again: the bits of a fresh handle once more
        calls = [call(*sp[0]), ("wait", lambda o, c, s: o.reset()), call(sp[0][0], sp[0][1], b=n)]
        one = np.stack([PM.shape32(taps, sps, x[r, :cuts[0]])[0] for r in range(2)])
        want = np.zeros((2, sps * 2 * n), np.complex64)
        want[:, :one.shape[1]] = one
        want[:, sps * n:sps * n + one.shape[1]] = one
    else:
        calls = [call(a, k) for a, k in sp]
        want = np.zeros((2, sps * 2 * n), np.complex64)
        want[:, :sps * n] = np.stack([PM.shape32(taps, sps, x[r])[0] for r in range(2)])
    return Row(name, "pulse", lambda: PulseShaper(sps=sps, max_streams=2, max_symbols=PulseShaper.TILE + 1, taps=taps),
               lambda o: NS(x=dev(x), y=zeros(2 * 2 * sps * 2 * n)), calls, lambda o, c: dict(out=host(c.y)), exact(out=want))


row("pulse", pulse_row)
row("pulse-other", pulse_row, sps=4)
row("pulse-reset", pulse_row, reset_after_first=True)


# ------------------------------------------------------------------ resamp
RESAMP_TAPS = np.random.default_rng(5).normal(size=7).astype(np.float32)


def resamp_row(name, rate=0.8, after_first=None):
    """after_first: None, "reset", "reset_phase" or "state" between the first call and the others"""
    nfilts = 2
    H = RM.geometry(nfilts, RESAMP_TAPS.size)[1]
    cuts = [max(H - 1, 1), H, int(Resampler.TILE / rate) + 50]
    n, step = sum(cuts), RM.step_of(rate)
    x = cplx(5, 2, n)
    cap = int(n * rate) + 8
    frac = np.array([1 << 31, 12345], np.uint32)

    def prep(o):
        return NS(x=dev(x), y=zeros(2 * 2 * cap), off=0, counts=[], said=[])

    def call(a, k):
        def f(o, c, s):
            n_out = o.work_device(p(c.x, a), n, k, 2, p(c.y, c.off), cap, s)
            c.counts.extend(n_out.tolist())
            c.off += int(n_out.max())
        return f

    def between(o, c, s):
        if after_first == "reset":
            o.reset()
            c.off = 0  # (the positions are zero again, and the next call writes over the first one's samples: they must be the same)
        elif after_first == "reset_phase":
            o.reset_phase(frac)
        else:
            c.said.extend(o.state().tolist())
        c.said.extend(o.produce(cuts[1], 2).tolist())  # the host mirror behind the entry

    calls = [call(a, k) for a, k in spans(cuts)]
    # the model, call by call: per stream the position, the history and where the samples go
    want = np.zeros((2, cap), np.complex64)
    acc, hist, off, counts, said = [0, 0], [None, None], 0, [], []
    seq = spans(cuts)
    if after_first is not None:
        calls.insert(1, ("wait", between))
        seq = [seq[0], None] + ([seq[0]] if after_first == "reset" else []) + seq[1:]
        if after_first == "reset":
            calls.insert(2, call(*spans(cuts)[0]))
    for item in seq:
        if item is None:
            if after_first == "reset":
                acc, hist, off = [0, 0], [None, None], 0
            elif after_first == "reset_phase":
                acc = [int(v) for v in frac]
            else:
                said.extend(acc)
            said.extend(RM.advance(acc[r], step, cuts[1])[0] for r in range(2))
            continue
        a, k = item
        outs = [RM.resample32(RESAMP_TAPS, nfilts, x[r, a:a + k], step, acc[r], hist[r]) for r in range(2)]
        for r, (y, h, ac) in enumerate(outs):
            want[r, off:off + y.size] = y
            hist[r], acc[r] = h, ac
            counts.append(y.size)
        off += max(y.size for y, _, _ in outs)
    return Row(name, "resamp", lambda: Resampler(nfilts, RESAMP_TAPS, rate, max_streams=2, max_samples=cuts[2]), prep, calls,
               lambda o, c: dict(out=host(c.y), counts=np.array(c.counts, np.int64), state=o.state(), said=np.array(c.said, np.uint64)),
               exact(out=want, counts=np.array(counts, np.int64), state=np.array(acc, np.uint64), said=np.array(said, np.uint64)))


row("resamp", resamp_row)
row("resamp-other", resamp_row, rate=2.5)
row("resamp-reset", resamp_row, after_first="reset")
row("resamp-reset_phase", resamp_row, after_first="reset_phase")
row("resamp-state", resamp_row, after_first="state")


# ------------------------------------------------------------------ ddc
DDC_TAPS = np.random.default_rng(6).normal(size=2).astype(np.float32)
DDC_INCS = (0.1, -0.2)


def ddc_mixed(z, inc):
    """what the rotator stage gives on the device for one whole stream: the mixer of model (a), as tests/test_ddc_gpu.py has it"""
    import torch
    rot = Rotator(inc)
    d_x, d_z = dev(z), zeros(2 * z.size)
    rot.work_device(d_x.data_ptr(), z.size, d_z.data_ptr(), T.stream())
    torch.cuda.synchronize()
    rot.close()
    return host(d_z).view(np.complex64)


def ddc_row(name, decim=3, swap=False, after_first=None):
    """decim 3, two taps, two channels on two inputs. swap: set_channel between the calls -- channel c reads input c, then 1 - c, then c
    again, all inside one hold (the table goes to the device on the stream of the next call). after_first: "reset" or "state"."""
    tile = min(capi.DDC_MAX_TILE, (capi.DDC_SPAN - (DDC_TAPS.size - 1)) // decim)
    cuts = [1, decim, tile * decim + 40]
    n = sum(cuts)
    x = cplx(6, 2, n)
    cap = n // decim + 4

    def make():
        o = Ddc(decim, DDC_TAPS, max_channels=2, max_inputs=2, max_samples=cuts[2])
        for ch, inc in enumerate(DDC_INCS):
            o.set_channel(ch, inc, input=ch)
        return o

    def prep(o):
        return NS(x=dev(x), y=zeros(2 * 2 * cap), off=0, counts=[], said=[])

    def call(a, k, inputs=None):
        def f(o, c, s):
            if inputs is not None:
                for ch, inc in enumerate(DDC_INCS):
                    o.set_channel(ch, inc, input=inputs[ch])
            n_out = o.work_device(p(c.x, a), n, k, 2, 2, p(c.y, c.off), cap, s)
            c.counts.append(n_out)
            c.off += n_out
        return f

    def between(o, c, s):
        if after_first == "reset":
            o.reset()
            c.off = 0
        else:
            c.said.extend(o.state().tolist())
        c.said.append(o.position())

    sp = spans(cuts)
    src = [[0, 1], [1, 0], [0, 1]] if swap else [[0, 1]] * 3  # src[call][channel]
    calls = [call(a, k, src[i] if swap else None) for i, (a, k) in enumerate(sp)]
    if after_first == "reset":
        calls = [calls[0], ("wait", between), call(*sp[0])] + calls[1:]
    elif after_first == "state":
        calls.insert(1, ("wait", between))

    def model(got):
        want = np.zeros((2, cap), np.complex64)
        phases, n_out = [], 0
        o = make()
        turns = [o.channel(ch)[1] for ch in range(2)]  # the increments in 2^-64 turns: the handle's own conversion, within 2 units of the exact one
        o.close()
        for t, inc in zip(turns, DDC_INCS):
            exact_t = ((K.turns(inc) + (1 << (K.FRAC - 65))) >> (K.FRAC - 64)) & ((1 << 64) - 1)
            assert min((t - exact_t) % (1 << 64), (exact_t - t) % (1 << 64)) <= 2
        for ch, inc in enumerate(DDC_INCS):
            z = np.concatenate([x[src[i][ch], a:a + k] for i, (a, k) in enumerate(sp)])  # the channel's own stream, whatever input it came from
            y = DM.decimate32(DDC_TAPS, decim, ddc_mixed(z, inc), 0, None)[0]
            want[ch, :y.size], n_out = y, y.size
            phases.append(DM.phase_after(0, turns[ch], n))
        counts = [DM.produce(a, decim, k) for a, k in sp]
        said = []
        if after_first == "reset":
            counts.insert(1, counts[0])
            said = [0]
        elif after_first == "state":
            said = [DM.phase_after(0, t, cuts[0]) for t in turns] + [cuts[0]]
        assert sum(counts[1 if after_first == "reset" else 0:]) == n_out
        exact(out=want, counts=np.array(counts, np.int64), state=np.array(phases, np.uint64), position=np.array([n], np.int64),
              said=np.array(said, np.uint64))(got)

    return Row(name, "ddc", make, prep, calls,
               lambda o, c: dict(out=host(c.y), counts=np.array(c.counts, np.int64), state=o.state(), position=np.array([o.position()], np.int64),
                                 said=np.array(c.said, np.uint64)), model)


row("ddc", ddc_row)
row("ddc-other", ddc_row, decim=5)
row("ddc-set_channel", ddc_row, swap=True)
row("ddc-reset", ddc_row, after_first="reset")
row("ddc-state", ddc_row, after_first="state")


# ------------------------------------------------------------------ spectrum: no state between calls, but one buffer of partial sums per handle
def spectrum_row(name):
    nfft = 64
    segs = [1, capi.SPECTRUM_CHUNK, capi.SPECTRUM_CHUNK + 1]
    cuts = [nfft * k for k in segs]
    cuts[2] += 5  # samples behind the last whole segment are not used
    n = sum(cuts)
    x = cplx(7, 2, n)

    def call(i, a, k):
        def f(o, c, s):
            c.rows.append(o.work_device(p(c.x, a), n, k, 2, p(c.y, i * nfft, 4), 3 * nfft, s))
        return f

    w, tw = spectrum_window("hann", nfft), spectrum_twiddles(nfft)
    want = np.stack([np.concatenate([SM.rows32(x[r, a:a + k], nfft, nfft, 0, w, tw, True) for a, k in spans(cuts)]) for r in range(2)])
    return Row(name, "spectrum", lambda: Spectrum(nfft, hop=nfft, avg=0, max_streams=2, max_samples=cuts[2]),
               lambda o: NS(x=dev(x), y=zeros(2 * 3 * nfft), rows=[]), [call(i, a, k) for i, (a, k) in enumerate(spans(cuts))],
               lambda o, c: dict(out=host(c.y), rows=np.array(c.rows, np.int32)), exact(out=want, rows=np.array([1, 1, 1], np.int32)))


row("spectrum", spectrum_row)


# ------------------------------------------------------------------ pfbch
def pfb_taps(ntaps):
    return np.random.default_rng(8).normal(size=ntaps).astype(np.float32)


def pfbch_row(name, M_=8, D=3, ntaps=40, sels=None, reset_after_first=False):
    """sels: the selection set in front of each call (A, B, A inside one hold), each a permutation of all channels"""
    taps = pfb_taps(ntaps)
    H = ntaps - 1
    tile = min(capi.PFBCH_MAX_TILE, (capi.PFBCH_SPAN - H - M_) // D)
    cuts = [H - 1, H, tile * D + 40]
    n = sum(cuts)
    x = cplx(8, 2, n)
    cap = n // D + 4
    sp = spans(cuts)
    use = [list(range(M_))] * 3 if sels is None else sels
    seq = [(a, k, use[i]) for i, (a, k) in enumerate(sp)]
    if reset_after_first:
        seq = [seq[0], None, seq[0]] + seq[1:]

    def prep(o):
        return NS(x=dev(x), y=zeros(2 * 2 * M_ * cap), off=0, counts=[], said=[])

    def call(a, k, sel):
        def f(o, c, s):
            if sels is not None:
                o.set_channels(sel)
            n_out = o.work_device(p(c.x, a), n, k, 2, p(c.y, c.off), cap, s)
            c.counts.append(n_out)
            c.off += n_out
        return f

    def reset(o, c, s):
        o.reset()
        c.off = 0
        c.said.append(o.position())

    calls = [("wait", reset) if item is None else call(*item) for item in seq]
    want = np.zeros((2, M_, cap), np.complex64)
    hist, pos, off, counts = [None, None], 0, 0, []
    for item in seq:
        if item is None:
            hist, pos, off = [None, None], 0, 0
            continue
        a, k, sel = item
        for r in range(2):
            y, hist[r] = CM.channelize32(taps, M_, D, x[r, a:a + k], pos, hist[r], sel)
            want[r, :, off:off + y.shape[1]] = y
        counts.append(y.shape[1])
        pos, off = pos + k, off + y.shape[1]
    return Row(name, "pfbch", lambda: PfbChannelizer(M_, D, taps, max_streams=2, max_samples=cuts[2]), prep, calls,
               lambda o, c: dict(out=host(c.y), counts=np.array(c.counts, np.int64), position=np.array([o.position()] + c.said, np.int64),
                                 channels=np.array(o.channels(), np.int32)),
               exact(out=want, counts=np.array(counts, np.int64), position=np.array([pos] + [0] * reset_after_first, np.int64),
                     channels=np.array(use[-1], np.int32)))


PERM_A, PERM_B = [0, 1, 2, 3, 4, 5, 6, 7], [5, 2, 7, 0, 3, 6, 1, 4]
row("pfbch", pfbch_row)
row("pfbch-other", pfbch_row, M_=16, D=8, ntaps=5)
row("pfbch-set_channels", pfbch_row, sels=[PERM_A, PERM_B, PERM_A])
row("pfbch-reset", pfbch_row, reset_after_first=True)


# ------------------------------------------------------------------ pfbsyn
def pfbsyn_row(name, M_=8, L=3, ntaps=40, sels=None, reset_after_first=False):
    taps = pfb_taps(ntaps)
    n_tail = YM.geometry(M_, L, ntaps)[0]
    tile = YM.tile(M_, L, ntaps)
    inst = -(-n_tail // L)  # instants the tail spans
    cuts = [max(inst - 1, 1), inst, tile + 7]
    n = sum(cuts)
    x = cplx(9, 2, M_, n)
    sp = spans(cuts)
    use = [list(range(M_))] * 3 if sels is None else sels
    seq = [(a, k, use[i]) for i, (a, k) in enumerate(sp)]
    if reset_after_first:
        seq = [seq[0], None, seq[0]] + seq[1:]

    def prep(o):
        return NS(x=dev(x), y=zeros(2 * 2 * n * L), off=0, counts=[], said=[])

    def call(a, k, sel):
        def f(o, c, s):
            if sels is not None:
                o.set_channels(sel)
            n_out = o.work_device(p(c.x, a), n, k, 2, p(c.y, c.off), n * L, s)
            c.counts.append(n_out)
            c.off += n_out
        return f

    def reset(o, c, s):
        o.reset()
        c.off = 0
        c.said.append(o.position())

    calls = [("wait", reset) if item is None else call(*item) for item in seq]
    want = np.zeros((2, n * L), np.complex64)
    tail, pos, off, counts = [None, None], 0, 0, []
    for item in seq:
        if item is None:
            tail, pos, off = [None, None], 0, 0
            continue
        a, k, sel = item
        for r in range(2):
            y, tail[r] = YM.synth32(taps, M_, L, x[r, :, a:a + k], pos, tail[r], sel)
            want[r, off:off + y.size] = y
        counts.append(k * L)
        pos, off = pos + k, off + k * L
    return Row(name, "pfbsyn", lambda: PfbSynthesizer(M_, L, taps, max_streams=2, max_samples=cuts[2]), prep, calls,
               lambda o, c: dict(out=host(c.y), counts=np.array(c.counts, np.int64), position=np.array([o.position()] + c.said, np.int64),
                                 channels=np.array(o.channels(), np.int32)),
               exact(out=want, counts=np.array(counts, np.int64), position=np.array([pos] + [0] * reset_after_first, np.int64),
                     channels=np.array(use[-1], np.int32)))


row("pfbsyn", pfbsyn_row)
row("pfbsyn-other", pfbsyn_row, M_=16, L=8, ntaps=5)
row("pfbsyn-set_channels", pfbsyn_row, sels=[PERM_A, PERM_B, PERM_A])
row("pfbsyn-reset", pfbsyn_row, reset_after_first=True)


# ------------------------------------------------------------------ symsync: one call, the caller's n_in array rewritten behind its back
def symsync_cfg():
    cfg, x = S.closed_set("lin-sps2")
    return cfg, x[:700]


def symsync_row(name, after=None):
    """after: None (the n_in case), "finish", "state" or "reset" right behind the call"""
    cfg, x = symsync_cfg()
    lens = [x.size, x.size - 33]
    n = x.size

    def prep(o):
        return NS(x=dev(np.stack([x, x[::-1].copy()])), y=zeros(2 * 2 * n), idx=zeros(2 * n, "int64"), mu=zeros(2 * n, "float64"),
                  n_in=np.array(lens, np.int32), said=[])

    def work(o, c, s):
        c.n_in[:] = lens
        rc = lib.dvbs2_symsync_work_device(o._h, p(c.x), n, c.n_in.ctypes.data, 2, p(c.y), n, n, p(c.idx), p(c.mu), s or None)
        c.n_in[:] = (2, 3)  # smaller legal counts, the moment the call returns
        assert rc == capi.OK

    def finish(o, c, s):
        v = [np.zeros(2, np.int32) for _ in range(3)]
        assert lib.dvbs2_symsync_finish(o._h, *[a.ctypes.data for a in v]) == capi.OK
        c.said.extend(np.concatenate(v).tolist())

    def state(o, c, s):
        st = o.state(1)
        c.said.extend([np.float64(st["mu"]).view(np.int64), st["n_read"]])

    def reset(o, c, s):
        o.reset()

    calls = [work] + ({"finish": [("wait", finish)], "state": [("wait", state)], "reset": [("wait", reset), work]}.get(after, []))
    bank = symsync_taps(cfg["sps"], cfg["rolloff"], cfg["rrc_delay"], cfg["n_subfilt"])
    ms = [S.SymSync(bank=bank, **cfg) for _ in range(2)]
    res = [m.work(xx) for m, xx in zip(ms, (x, x[::-1][:lens[1]]))]
    out, idx, mu = np.zeros((2, n), np.complex64), np.zeros((2, n), np.int64), np.zeros((2, n), np.float64)
    for r, (o_, i_, m_, _, _) in enumerate(res):
        out[r, :o_.size], idx[r, :i_.size], mu[r, :m_.size] = o_, i_, m_
    fin = [res[0][0].size, res[1][0].size, res[0][3], res[1][3], res[0][4], res[1][4]]
    said = {"finish": fin, "state": [np.float64(ms[1].state()["mu"]).view(np.int64), ms[1].state()["n_read"]]}.get(after, [])

    def collect(o, c):
        v = [np.zeros(2, np.int32) for _ in range(3)]
        assert lib.dvbs2_symsync_finish(o._h, *[a.ctypes.data for a in v]) == capi.OK
        st = [o.state(r) for r in range(2)]
        return dict(out=host(c.y), idx=host(c.idx), mu=host(c.mu), finish=np.concatenate(v), said=np.array(c.said, np.int64),
                    state=np.array([[np.float64(t[k]).view(np.int64) for k in ("vi", "cnt", "mu")] + [t["n_read"], t["jump"], t["init"], t["status"]] for t in st], np.int64))

    wstate = np.array([[np.float64(m.state()[k]).view(np.int64) for k in ("vi", "cnt", "mu")] + [m.state()[k] for k in ("n_read", "jump", "init", "status")]
                       for m in ms], np.int64)
    return Row(name, "symsync", lambda: SymbolSync(max_streams=2, max_samples=n, **cfg), prep, calls, collect,
               exact(out=out, idx=idx, mu=mu, finish=np.array(fin, np.int32), said=np.array(said, np.int64), state=wstate))


row("symsync", symsync_row)
row("symsync-finish", symsync_row, "finish")
row("symsync-state", symsync_row, "state")
row("symsync-reset", symsync_row, "reset")


# ------------------------------------------------------------------ rotator: the host mirror (counter, phase, queue) advances at enqueue time
def rotator_row(name):
    cuts, inc = [100, 100, 37], 0.0371
    n = sum(cuts)
    x = cplx(10, n)
    ups = [(150, -0.02), (201, 0.3)]  # inside the second call, and one sample into the third

    def make():
        o = Rotator(inc)
        o.schedule(*ups[0])
        return o

    def call(i, a, k):
        def f(o, c, s):
            if i == 1:
                o.schedule(*ups[1])  # queued while the first call is pending
            o.work_device(p(c.x, a), k, p(c.y, a), s)
        return f

    def model(got):
        m = K.Rotator(inc)
        for u in ups:
            m.schedule(*u)
        want, bound = m.work(x)
        err = np.abs(got["out"].view(np.complex64).astype(np.complex128) - want)
        print(f"rotator: worst error / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all() and got["position"].tolist() == [n, 0]

    return Row(name, "rotator", make, lambda o: NS(x=dev(x), y=zeros(2 * n)), [call(i, a, k) for i, (a, k) in enumerate(spans(cuts))],
               lambda o, c: dict(out=host(c.y), position=np.array(o.position(), np.int64)), model)


row("rotator", rotator_row)


# ------------------------------------------------------------------ the PL receive stages on one raw stream of nine 36-slot frames
PL_PLSC = P.plsc_of(24, 1, 1)  # 32APSK 3/4 short with pilots: 36 slots
PL_FRAMES, PL_GOLD, PL_MAXF = 9, 0, 16


@functools.lru_cache(None)
def pl_stream():
    x, sofs, _ = P.make_stream([PL_PLSC] * PL_FRAMES, 21, offset=1400, gold=PL_GOLD, tail=100)
    assert x.size <= PlSync.MIN_SYMBOLS
    x.setflags(write=False)
    return x, sofs


def records(t):
    return host(t).view(PlSync.FRAME_DTYPE)


@functools.lru_cache(None)
def pl_tracked():
    """plsync_model's tracker over the whole stream from a reset: (records, consumed, state, the metric's bound per index)"""
    x, _ = pl_stream()
    met, bound = P.metric(x)
    log = []
    recs, consumed, state, visits = P.track(met, P.make_decoder(x, log=log), 3, -1, PL_MAXF)
    assert P.guard(dict(met=met, bound=bound, visits=visits, log=log)) == (0, 0)  # no decision of the model within float32 rounding of a threshold or a tie
    return recs, consumed, state, bound


def plsync_model(last_start=0):
    """The records, the count, `consumed` and the state of the search that ended the row are the model tracker's: sof_index, plsc and
    flags equal, the metric within the model's float32 bound (as compare_records of tests/test_plsync_gpu.py), the bytes behind the
    last record untouched. last_start: where the last call's buffer begins in the stream (`consumed` counts from there)."""
    def check(got):
        _, sofs = pl_stream()
        want, consumed, state, bound = pl_tracked()
        assert [r[0] for r in want] == sofs and len(want) == PL_FRAMES  # the model finds the frames the stream was made of
        recs = got["records"].view(PlSync.FRAME_DTYPE)
        assert not got["records"][16 * PL_FRAMES:].any() and not recs["reserved"].any()
        recs = recs[:PL_FRAMES]
        assert recs["sof_index"].tolist() == [r[0] for r in want] and recs["plsc"].tolist() == [r[2] for r in want]
        assert recs["flags"].tolist() == [r[3] for r in want]
        at = np.array([r[0] + 89 for r in want])
        err = np.abs(recs["metric"].astype(np.float64) - np.array([r[1] for r in want]))
        print(f"plsync: metric worst error / bound {np.max(err / bound[at]):.3f}")
        assert (err <= bound[at]).all()
        assert got["finish"].tolist()[-3:] == [PL_FRAMES, consumed - last_start, state] and state == capi.PLSYNC_LOCKED
    return check


def plsync_row(name, after=None):
    """three searches cut where the tracker consumes all it was given (no frame is complete before the third); after: "finish" or
    "reset" behind the first"""
    x, sofs = pl_stream()
    cuts = [517, 583, x.size - 1100]  # the first header ends at 1489

    def prep(o):
        return NS(x=dev(x), rec=zeros(PL_MAXF * 16, "uint8"), said=[])

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, a), k, p(c.rec), s)

    def finish(o, c, s):
        c.said.extend(o.finish())

    def reset(o, c, s):
        o.reset()

    sp = spans(cuts)
    if after == "reset":  # a search, the reset, then the whole stream from its start: the records of a fresh handle
        calls = [call(*sp[0]), ("wait", reset), call(0, x.size)]
    elif after == "finish":
        calls = [call(*sp[0]), ("wait", finish)] + [call(a, k) for a, k in sp[1:]]
    else:
        calls = [call(a, k) for a, k in sp]

    def collect(o, c):
        return dict(records=host(c.rec), finish=np.array(c.said + list(o.finish()), np.int32))

    def model(got):
        plsync_model(0 if after == "reset" else sp[2][0])(got)
        if after == "finish":
            assert got["finish"].tolist()[:3] == [0, cuts[0], capi.PLSYNC_SEARCHING]
    return Row(name, "plsync", lambda: PlSync(plsc=-1, max_symbols=PlSync.MIN_SYMBOLS, max_frames=PL_MAXF), prep, calls, collect, model)


row("plsync", plsync_row)
row("plsync-finish", plsync_row, "finish")
row("plsync-reset", plsync_row, "reset")


def pl_chain_row(name):
    """search -> gather (n_frames = max_frames: the device count bounds it) -> coarse estimate on the records -> front end, no host read
    in between; the host knows the counts from how the stream was made"""
    x, sofs = pl_stream()
    L = M.pls_parse(PL_PLSC)["plframe_len"]
    cnt = PL_FRAMES - 1  # the tracker locks at the second header

    def make():
        return (PlSync(plsc=-1, max_symbols=PlSync.MIN_SYMBOLS, max_frames=PL_MAXF), PlCoarse(1, -1, max_frames=PL_MAXF),
                PlFrontEnd(PL_GOLD, PL_PLSC, max_frames=cnt))

    def prep(o):
        fe = o[2]
        return NS(x=dev(x), rec=zeros(PL_MAXF * 16, "uint8"), fr=zeros(2 * (cnt * L + 90)), cnt=zeros(1, "int32"), fo=zeros(PL_MAXF),
                  cc=zeros(PL_MAXF, "int32"), ne=zeros(PL_MAXF, "int32"), xfec=zeros(2 * cnt * fe.xfecframe_len), plsc=zeros(cnt, "uint8"),
                  ph=zeros(cnt))

    calls = [lambda o, c, s: o[0].work_device(p(c.x), x.size, p(c.rec), s),
             lambda o, c, s: o[0].gather_device(p(c.x), p(c.rec), PL_MAXF, PL_PLSC, p(c.fr), p(c.cnt), s),
             lambda o, c, s: o[1].work_records_device(p(c.x), x.size, 0, p(c.rec), PL_FRAMES, p(c.fo), p(c.cc), p(c.ne), s),
             # the coarse_corrected flags of frames 1.. are those of the gathered (locked) frames
             lambda o, c, s: o[2].work_device(p(c.fr), cnt, 1, p(c.cc, 1, 4), p(c.fo, 1, 4), p(c.xfec), s, plsc_decoded=p(c.plsc), plheader_phase=p(c.ph))]

    def collect(o, c):
        return dict(records=host(c.rec), finish=np.array(o[0].finish(), np.int32), frames=host(c.fr), count=host(c.cnt), foffset=host(c.fo),
                    corrected=host(c.cc), new_est=host(c.ne), xfec=host(c.xfec), plsc=host(c.plsc), phase=host(c.ph))

    def model(got):
        plsync_model()(got)
        assert got["count"].tolist() == [cnt] and got["plsc"].tolist() == [PL_PLSC] * cnt
        want = np.concatenate([x[sofs[1]:sofs[1] + cnt * L], x[sofs[1] + cnt * L:sofs[1] + cnt * L + 90]])
        assert raw(got["frames"]) == raw(want), "the gathered frames are not the stream's"
        assert got["new_est"].tolist()[:PL_FRAMES] == [1] * PL_FRAMES and got["corrected"].tolist()[:PL_FRAMES] == [1] * PL_FRAMES  # no carrier offset
        assert (np.abs(got["foffset"][:PL_FRAMES]) < 3.3875e-4).all()  # (a clean stream: every estimate is within the flag's own limit)

    return Row(name, ("plsync", "plcoarse", "plframe"), make, prep, calls, collect, model)


row("pl-chain", pl_chain_row)


def plcoarse_row(name, reset_after_first=False):
    """frames 1 + 2 + 3 of rotated headers in three calls, period 2: a window straddles every call boundary, and the first estimate
    (1e-4, inside the corrected range) switches the handle from the SOF form to the full PLHEADER. The expected values are
    plcoarse_model's over the same frames in the same order, its state restarted at the reset: new_est and coarse_corrected equal,
    coarse_foffset within the model's float32 bound of the estimate in force (as compare of tests/test_plcoarse_gpu.py)."""
    f = 1e-4
    cuts = [1, 2, 3]
    nf = sum(cuts)
    hdrs = np.stack([K.rotated_header(PL_PLSC, f, 0.3 * i) for i in range(nf)]).astype(np.complex64)
    plscs = np.full(nf, PL_PLSC, np.uint8)
    sp = spans(cuts)
    seq = [sp[0], None, sp[0], sp[1]] if reset_after_first else sp

    def prep(o):
        return NS(x=dev(hdrs), plsc=dev(plscs), fo=zeros(nf), cc=zeros(nf, "int32"), ne=zeros(nf, "int32"))

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, 90 * a), 90, k, p(c.plsc, a, 1), p(c.fo, a, 4), p(c.cc, a, 4), p(c.ne, a, 4), s)

    calls = [("wait", lambda o, c, s: o.reset()) if it is None else call(*it) for it in seq]

    def model(got):
        # what each output slot holds in the end: the last call that wrote it (behind a reset the first frame is written again)
        fo, cc, ne, bound = np.zeros(nf), np.zeros(nf, np.int32), np.zeros(nf, np.int32), np.zeros(nf)
        state, in_force, windows = K.Coarse(2), 0.0, 0
        for it in seq:
            if it is None:
                state, in_force = K.Coarse(2), 0.0
                continue
            a, k = it
            m = K.run(hdrs[a:a + k], plscs[a:a + k], 2, state=state)
            assert m["eligible"].all()  # no decision of the model within float32 rounding of a limit
            for j in range(k):
                if m["new_est"][j]:
                    in_force, windows = m["bound"][j], windows + 1
                fo[a + j], cc[a + j], ne[a + j], bound[a + j] = m["foffset"][j], m["corrected"][j], m["new_est"][j], in_force
        err = np.abs(got["foffset"].astype(np.float64) - fo)
        print(f"{name}: {windows} windows, estimates {got['foffset']}, largest error {err.max():.2e}, largest bound {bound.max():.2e}")
        assert (err <= bound).all() and windows >= 1
        assert got["new_est"].tolist() == ne.tolist() and got["corrected"].tolist() == cc.tolist()
        if not reset_after_first:
            assert cc.tolist() == [0, 1, 1, 1, 1, 1] and abs(fo[-1] - f) < 1e-6  # the run covers the change of form

    return Row(name, "plcoarse", lambda: PlCoarse(2, -1, max_frames=4), prep, calls,
               lambda o, c: dict(foffset=host(c.fo), corrected=host(c.cc), new_est=host(c.ne)), model)


row("plcoarse", plcoarse_row)
row("plcoarse-reset", plcoarse_row, reset_after_first=True)


def plpayload_row(name):
    """frames 1 + 2 + 1 of one handle in three calls; the expected symbols are the CPU oracle's (oracle/pl_oracle.c) under the bound of
    tests/test_bch_demap_gpu.py: 4e-4, a float rotator recurrence against the direct phase on symbols of magnitude up to about 4"""
    nf, cuts = 4, [1, 2, 1]
    rng = np.random.default_rng(12)
    info = pls_parse(PL_PLSC)  # 36 slots with pilots
    n_pay, n_x, n_pil = info["payload_len"], info["xfecframe_len"], max(info["n_pilots"], 1)
    pay = cplx(12, nf, n_pay)
    ph, fo = rng.uniform(-3, 3, nf).astype(np.float32), rng.uniform(-1e-4, 1e-4, nf).astype(np.float32)
    cc, pp = np.ones(nf, np.int32), rng.uniform(-3, 3, (nf, n_pil)).astype(np.float32)
    inc = np.ascontiguousarray(2.0 * np.pi * fo.astype(np.float64), np.float32)  # the entry takes the phase increment per symbol

    def prep(o):
        return NS(pay=dev(pay), ph=dev(ph), fo=dev(inc), cc=dev(cc), pp=dev(pp), y=zeros(2 * nf * n_x))

    def call(a, k):
        def f(o, c, s):
            capi.check(lib.dvbs2_plpayload_process_device(o._h, p(c.pay, a * n_pay), k, p(c.ph, a, 4), p(c.fo, a, 4), p(c.cc, a, 4),
                                                          p(c.pp, a * n_pil, 4), p(c.y, a * n_x), s or None))
        return f

    def model(got):
        want = T.oracle_pl_payload(pay, 36, True, 0, ph, fo, cc, pp)
        err = np.abs(got["out"].view(np.complex64).reshape(nf, n_x) - want).max()
        print(f"plpayload: worst distance from the oracle {err:.2e}")
        assert err < 4e-4

    return Row(name, "plpayload", lambda: PlPayload(gold_code=0, n_slots=36, has_pilots=True, max_frames=2), prep,
               [call(a, k) for a, k in spans(cuts)], lambda o, c: dict(out=host(c.y)), model)


row("plpayload", plpayload_row)


# ------------------------------------------------------------------ the transmit chain: bbframer -> enc -> plframer, device-resident
TX_PLSC = P.plsc_of(1, 1, 1)  # QPSK 1/4 short with pilots


def ts_packets(n, key):
    ts = np.random.default_rng([14, key]).integers(0, 256, (n, 188)).astype(np.uint8)
    ts[:, 0] = 0x47
    return ts


def bbframer_row(name, between=None):
    """frames 1 + 2 + 1; between: "reset" (stream-ordered: reset, then a call, both pending) or "counters" (synchronises the stream)"""
    kb = FEC["bch_k"] // 8
    cuts = [1, 2, 1]
    ts = ts_packets(4 * (kb // 188 + 2), 1)
    m = BM.BbFramerModel(8 * kb)
    seq = [(a, k) for a, k in spans(cuts)]
    if between == "reset":
        seq = [seq[0], None] + seq
    elif between == "counters":
        seq = [seq[0], None] + seq[1:]
    want, said, rd, fr = np.zeros((5, kb), np.uint8), [], 0, 0
    plan = []
    for it in seq:
        if it is None:
            if between == "reset":
                m.reset()
                rd = 0
            else:
                said.extend(m.counters().values())
            plan.append(None)
            continue
        out = m.work(ts.reshape(-1)[188 * rd:], it[1])
        want[fr:fr + it[1]] = out
        plan.append((rd, it[1], fr))
        rd, fr = rd + m.packets_read, fr + it[1]

    def prep(o):
        return NS(ts=dev(ts), y=zeros(5 * kb, "uint8"), said=[])

    def call(rd_, k, fr_):
        return lambda o, c, s: o.work_device(p(c.ts, rd_, 188), k, p(c.y, fr_ * kb, 1), 0, s)

    def mid(o, c, s):
        if between == "reset":
            o.reset(s)
        else:
            c.said.extend(o.counters(s).values())

    calls = [((("wait" if between == "counters" else "call"), mid)) if it is None else call(*it) for it in plan]
    return Row(name, "bbframer", lambda: BbFramer(framesize=SHORT, rate="C1_4", max_frames=2), prep, calls,
               lambda o, c: dict(out=host(c.y), said=np.array(c.said, np.uint64), counters=np.array(list(o.counters().values()), np.uint64)),
               exact(out=want, said=np.array(said, np.uint64), counters=np.array(list(m.counters().values()), np.uint64)))


row("bbframer", bbframer_row)
row("bbframer-reset", bbframer_row, "reset")
row("bbframer-counters", bbframer_row, "counters")


def enc_model(msg, got):
    N, Kl, _, _ = T.ldpc_info(TABLE)
    bch = np.unpackbits(got["bch_cw"].reshape(msg.shape[0], -1), axis=1)
    assert bch.shape[1] == Kl and raw(got["bch_cw"].reshape(msg.shape[0], -1)[:, :msg.shape[1]]) == raw(msg), "the BCH codeword is not systematic"
    assert raw(np.unpackbits(got["ldpc_cw"].reshape(msg.shape[0], -1), axis=1)) == raw(T.ldpc_encode(TABLE, bch)), "LDPC: not the restated encoder's word"
    bits = np.unpackbits(got["ldpc_cw"].reshape(msg.shape[0], -1), axis=1).reshape(msg.shape[0], -1, 2)
    want = ((1.0 - 2.0 * bits[..., 0]) + 1j * (1.0 - 2.0 * bits[..., 1])) * np.sqrt(0.5)  # EN 302 307-1 figure 9
    assert np.abs(got["syms"].view(np.complex64).reshape(msg.shape[0], -1) - want).max() < 1e-6


def enc_row(name):
    cuts = [1, 2, 1]
    nb, bn, ln, ns = FEC["bch_k"] // 8, FEC["bch_n"] // 8, FEC["ldpc_n"] // 8, FEC["ldpc_n"] // 2
    msg = np.random.default_rng(15).integers(0, 256, (4, nb)).astype(np.uint8)

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, a * nb, 1), k, p(c.bch, a * bn, 1), p(c.ldpc, a * ln, 1), p(c.syms, a * ns), s)

    return Row(name, "enc", lambda: FecEncoder(framesize=SHORT, rate="C1_4", constellation=QPSK, max_frames=2),
               lambda o: NS(x=dev(msg), bch=zeros(4 * bn, "uint8"), ldpc=zeros(4 * ln, "uint8"), syms=zeros(2 * 4 * ns)),
               [call(a, k) for a, k in spans(cuts)], lambda o, c: dict(bch_cw=host(c.bch), ldpc_cw=host(c.ldpc), syms=host(c.syms)),
               functools.partial(enc_model, msg))


row("enc", enc_row)


def plframer_row(name):
    """frames 1 + 2 + 1 of a set sequence of four: each call frames the first n of the sequence, so calls of 1, 3 and 4 frames"""
    seq = [TX_PLSC, P.plsc_of(0, 0, 0), TX_PLSC, TX_PLSC]  # a dummy frame among them
    lay = F.layout(seq)
    data = F.planted_data(np.random.default_rng(16), lay["in_syms"])
    total = lay["out_syms"] + 90

    def make():
        o = PlFramer(PL_GOLD, max_frames=4)
        o.set_sequence(seq)
        return o

    def call(i, nfr):
        return lambda o, c, s: o.work_device(p(c.x), nfr, seq[nfr - 1], p(c.y, i * total), s)

    def model(got):
        out = got["out"].reshape(3, total, 2)
        for i, nfr in enumerate((1, 3, 4)):
            w = F.frames(seq[:nfr], PL_GOLD, data[:F.layout(seq[:nfr])["in_syms"]], seq[nfr - 1])
            assert raw(out[i, :w.shape[0]]) == raw(w) and not out[i, w.shape[0]:].any(), nfr

    return Row(name, "plframer", make, lambda o: NS(x=dev(np.ascontiguousarray(data, np.float32).reshape(-1)), y=zeros(2 * 3 * total)),
               [call(i, nfr) for i, nfr in enumerate((1, 3, 4))], lambda o, c: dict(out=host(c.y)), model)


row("plframer", plframer_row)


def tx_chain_row(name):
    """bbframer -> enc -> plframer on device buffers, twice two frames, nothing read on the host in between"""
    seq = [TX_PLSC, TX_PLSC]
    lay = F.layout(seq)
    nb, ns = FEC["bch_k"] // 8, FEC["ldpc_n"] // 2
    ts = ts_packets(4 * (nb // 188 + 2), 2)
    total = lay["out_syms"] + 90
    m = BM.BbFramerModel(8 * nb)
    reads = []
    bb = []
    for _ in range(2):
        rd = sum(r for r in reads)
        bb.append(m.work(ts.reshape(-1)[188 * rd:], 2))
        reads.append(m.packets_read)

    def make():
        fr = PlFramer(PL_GOLD, max_frames=2)
        fr.set_sequence(seq)
        return (BbFramer(framesize=SHORT, rate="C1_4", max_frames=2), FecEncoder(framesize=SHORT, rate="C1_4", constellation=QPSK, max_frames=2), fr)

    def prep(o):
        return NS(ts=dev(ts), bb=zeros(4 * nb, "uint8"), syms=zeros(2 * 4 * ns), ldpc=zeros(4 * o[1].ldpc_n // 8, "uint8"),
                  bch=zeros(4 * o[1].bch_n // 8, "uint8"), y=zeros(2 * 2 * total))

    def stage(i):
        rd = sum(reads[:i])
        return [lambda o, c, s: o[0].work_device(p(c.ts, rd, 188), 2, p(c.bb, 2 * i * nb, 1), 0, s),
                lambda o, c, s: o[1].work_device(p(c.bb, 2 * i * nb, 1), 2, p(c.bch, 2 * i * o[1].bch_n // 8, 1), p(c.ldpc, 2 * i * o[1].ldpc_n // 8, 1),
                                                 p(c.syms, 2 * i * ns), s),
                lambda o, c, s: o[2].work_device(p(c.syms, 2 * i * ns), 2, seq[-1], p(c.y, i * total), s)]

    def model(got):
        assert raw(got["bbframes"]) == raw(np.concatenate(bb)), "the BBFRAMEs are not the model's"
        enc_model(np.concatenate(bb), got)
        syms = got["syms"].reshape(2, lay["in_syms"], 2)
        for i in range(2):
            assert raw(got["out"].reshape(2, total, 2)[i]) == raw(F.frames(seq, PL_GOLD, syms[i], seq[-1])), "the PLFRAMEs are not the model's of the encoder's symbols"

    return Row(name, ("bbframer", "enc", "plframer"), make, prep, stage(0) + stage(1),
               lambda o, c: dict(bbframes=host(c.bb), bch_cw=host(c.bch), ldpc_cw=host(c.ldpc), syms=host(c.syms), out=host(c.y)), model)


row("tx-chain", tx_chain_row)


# ------------------------------------------------------------------ the FEC receive stages
def bbdeheader_row(name, between=None):
    """frames 1 + 2 + 1 (a TS packet straddles every boundary); between: "reset" (stream-ordered, nothing waits) or "state": the
    counters and the byte count read on the stream (both synchronise it)"""
    kb = FEC["bch_k"] // 8
    per = kb + 2 * 188  # room per frame: above what a DATAFIELD and a carried partial packet give
    kbch = 8 * kb
    frames = T.bbframe_stream(kbch, 4, T.ts_up_stream(4 * (-(-(kbch - 80) // (8 * 188))) + 1, np.random.default_rng(17)), 0)
    sp = spans([1, 2, 1])
    seq = {"reset": [sp[0], None] + sp, "state": [sp[0], None] + sp[1:]}.get(between, sp)

    def prep(o):
        return NS(x=dev(frames), y=zeros(5 * per, "uint8"), said=[], slot=0)

    def call(a, k):
        def f(o, c, s):
            o.work_device(p(c.x, a * kb, 1), k, p(c.y, c.slot * per, 1), s)
            c.slot += k
        return f

    def mid(o, c, s):
        if between == "reset":
            o.reset(s)
        else:
            c.said.extend(list(o.counters(s).values()) + [o.finish(s)])

    calls = [(("wait" if between == "state" else "call"), mid) if it is None else call(*it) for it in seq]

    def model(got):
        m, said, slot = T.OracleBbDeheader(kbch), [], 0
        want = np.zeros(5 * per, np.uint8)
        last = 0
        for it in seq:
            if it is None:
                if between == "reset":
                    m = T.OracleBbDeheader(kbch)
                else:
                    said = list(m.counters().values()) + [last]
                continue
            ts = m.work(frames[it[0]:it[0] + it[1]])
            want[slot * per:slot * per + ts.size] = ts
            last, slot = ts.size, slot + it[1]
        exact(out=want, said=np.array(said, np.int64), counters=np.array(list(m.counters().values()), np.int64), produced=np.array([last], np.int64))(got)

    return Row(name, "bbdeheader", lambda: BbDeheader(framesize=SHORT, rate="C1_4", max_frames=2), prep, calls,
               lambda o, c: dict(out=host(c.y), said=np.array(c.said, np.int64), produced=np.array([o.finish()], np.int64),
                                 counters=np.array(list(o.counters().values()), np.int64)), model)


row("bbdeheader", bbdeheader_row)
row("bbdeheader-reset", bbdeheader_row, "reset")
row("bbdeheader-state", bbdeheader_row, "state")


def bch_row(name):
    """frames 1 + 2 + 1 of the all-zero codeword with 1, 2, 3 and 0 planted errors: the message is zeros, the count the planted one"""
    nb, kb = FEC["bch_n"] // 8, FEC["bch_k"] // 8
    cw = np.zeros((4, nb), np.uint8)
    rng = np.random.default_rng(18)
    planted = [1, 2, 3, 0]
    for f, t in enumerate(planted):
        for pos in rng.choice(8 * nb, t, replace=False):
            cw[f, pos // 8] ^= 0x80 >> (pos % 8)

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, a * nb, 1), k, p(c.msg, a * kb, 1), p(c.corr, a, 4), s)

    return Row(name, "bch", lambda: BchDecoder(framesize=SHORT, rate="C1_4", max_frames=2),
               lambda o: NS(x=dev(cw), msg=zeros(4 * kb, "uint8") + 0x5A, corr=zeros(4, "int32") - 7),
               [call(a, k) for a, k in spans([1, 2, 1])], lambda o, c: dict(msg=host(c.msg), corr=host(c.corr)),
               exact(msg=np.zeros(4 * kb, np.uint8), corr=np.array(planted, np.int32)))


row("bch", bch_row)


def demap_row(name):
    ns, nl = FEC["ldpc_n"] // 2, FEC["ldpc_n"]
    syms = cplx(19, 4, ns)
    n0 = np.array([0.3, 0.5, 0.2, 0.9], np.float32)

    def call(a, k):
        return lambda o, c, s: o.work_device(p(c.x, a * ns), k, p(c.n0, a, 4), k, p(c.y, a * nl, 1), s)

    return Row(name, "demap", lambda: Demapper(framesize=SHORT, rate="C1_4", constellation=QPSK, max_frames=2),
               lambda o: NS(x=dev(syms), n0=dev(n0), y=zeros(4 * nl, "int8")), [call(a, k) for a, k in spans([1, 2, 1])],
               lambda o, c: dict(out=host(c.y)), exact(out=T.oracle_demap(syms, n0, 4)))


row("demap", demap_row)


def demap_table_row(name):
    """a caller's table (tests/demap_table_model.py): frames 1 + 2 of its case, then frame 0 again with the one N0"""
    _, table, framesize, column = DT.CASES[-1]
    syms, nat_pf, nat_one, pts, p32, one_n0 = DT.demap_case(table, framesize)
    n_mod = int(np.log2(len(pts)))
    col = DT.natural(n_mod) if column is None else list(column)
    want_pf, want_one = DT.permute_columns(nat_pf, n_mod, col), DT.permute_columns(nat_one, n_mod, col)
    ns = syms.shape[1]
    nl = ns * n_mod
    n0 = np.concatenate([DT.N0_FRAMES, [one_n0]]).astype(np.float32)
    calls = [lambda o, c, s: o.work_device(p(c.x), 1, p(c.n0, 0, 4), 1, p(c.y, 0, 1), s),
             lambda o, c, s: o.work_device(p(c.x, ns), 2, p(c.n0, 1, 4), 2, p(c.y, nl, 1), s),
             lambda o, c, s: o.work_device(p(c.x), 1, p(c.n0, 3, 4), 1, p(c.y, 3 * nl, 1), s)]
    return Row(name, "demap", lambda: Demapper.from_table(framesize, p32, column, max_frames=2),
               lambda o: NS(x=dev(np.array(syms)), n0=dev(n0), y=zeros(4 * nl, "int8")), calls, lambda o, c: dict(out=host(c.y)),
               exact(out=np.concatenate([want_pf, want_one[:1]])))


row("demap_table", demap_table_row)


# ================================================================== the tests
# handle types whose side-stream behaviour has its own test elsewhere instead of a row here
ELSEWHERE = {"ldpc": "tests/test_ldpc_gpu.py: the enqueue / finish tests on a side stream", "chain": "tests/test_ldpc_gpu.py, tests/test_enc_gpu.py: enqueue_device on a side stream",
             "plsync_batch": "tests/test_plsync_batch_stream_gpu.py: its rows, by this file's machinery", "plcoarse_batch": "tests/test_plsync_batch_stream_gpu.py: its rows, by this file's machinery"}
# every entry whose header comment says "waits" or "synchronous" and that may be called while work is pending -> its row
WAITING = {"agc reset": "agc-reset", "agc set_gain": "agc-set_gain", "agc state": "agc-state", "symsync reset": "symsync-reset",
           "symsync state": "symsync-state", "symsync finish": "symsync-finish", "pulse reset": "pulse-reset", "resamp reset": "resamp-reset",
           "resamp reset_phase": "resamp-reset_phase", "resamp state": "resamp-state", "ddc reset": "ddc-reset", "ddc state": "ddc-state",
           "pfbch reset": "pfbch-reset", "pfbsyn reset": "pfbsyn-reset", "plcoarse reset": "plcoarse-reset", "plsync finish": "plsync-finish",
           "plsync reset": "plsync-reset", "bbframer counters": "bbframer-counters", "bbframer reset": "bbframer-reset",
           "bbdeheader state": "bbdeheader-state", "bbdeheader reset": "bbdeheader-reset"}
STAGES = ["agc", "awgn", "iqconv", "pulse", "resamp", "ddc", "spectrum", "pfbch", "pfbsyn", "symsync", "rotator", "plsync", "plcoarse",
          "pl-chain", "plpayload", "plframer", "bbframer", "bbdeheader", "enc", "bch", "demap", "demap_table"]
PAIRS = [("agc", "agc-other"), ("pulse", "pulse-other"), ("resamp", "resamp-other"), ("ddc", "ddc-other"), ("pfbch", "pfbch-other"),
         ("pfbsyn", "pfbsyn-other")]


def handles_of(r):
    return set(r.handle if isinstance(r.handle, tuple) else (r.handle,))


def test_every_stage_has_its_row():
    """every handle type of capi -- what has a dvbs2_<type>_destroy -- has a row, or names the test that holds its side-stream case"""
    types = {name[len("dvbs2_"):-len("_destroy")] for name in capi.SYMBOLS if name.endswith("_destroy")}
    rows = {name: get_row(name) for name in ROWS}
    covered = set().union(*(handles_of(r) for r in rows.values()))
    assert covered | set(ELSEWHERE) == types and not covered & set(ELSEWHERE), (sorted(types - covered - set(ELSEWHERE)), sorted(covered - types))
    assert set(STAGES) <= set(ROWS) and set(WAITING.values()) <= set(ROWS)
    assert all(rows[name].waits or name in ("bbframer-reset", "bbdeheader-reset") for name in WAITING.values())  # the two stream-ordered resets wait for nothing
    assert all(r.model is not None for r in rows.values()), "a row whose serialized pass is tied to no model"


def test_the_hold_holds():
    """The fixture itself: a side stream is not ordered behind the held null stream, and a hold lasts at least half its length."""
    import torch
    cal = T.sleep_calibration()
    side, null = T.side_stream(), T.null_stream()
    d = zeros(1024, "int32")
    torch.cuda.synchronize()
    T.hold(null, 50.0)
    with torch.cuda.stream(side):
        d.fill_(7)
    side.synchronize()
    still = T.pending(null)
    torch.cuda.synchronize()
    assert still, "the null stream had drained: the fill on the side stream waited for it, or the hold was too short"
    assert (host(d) == 7).all()
    for ms in (T.HOLD_MIN_MS, 100.0):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        T.hold(side, ms)
        b.record(side)
        side.synchronize()
        took = a.elapsed_time(b)
        print(f"stream-order: calibration {cal['cycles_per_ms']:.0f} cycles per ms ({cal['probe_cycles']} cycles in {cal['probe_ms']:.3f} ms); a hold of {ms:.0f} ms lasted {took:.2f} ms")
        assert took >= ms / 2


@pytest.mark.parametrize("size", [712, 1 << 20])
def test_runtime_memset_is_complete_behind_a_null_stream_wait(size):
    """What every constructor and reset relies on (memset_done of csrc/device_stage.h): hipMemset of device memory followed by a wait
    for the null stream has written its pattern when that returns -- read back over a side stream that waits for nothing, with the
    null stream held when the fill is called. hipMemset ALONE does not give that on this runtime: it returns at once and the fill runs
    behind the hold (at 1 MiB every time it was tried, at 712 bytes every time but the first fill of a process); that raw observation
    is printed for notes/stream_order.md and is the reason the library waits. Sizes: the two histories of plsync, and a megabyte.
    test_a_handle_created_while_the_null_stream_is_busy checks the same through the library's own constructors."""
    import torch
    rt = T.hip_runtime()
    side, null = T.side_stream(), T.null_stream()
    d = zeros(size, "uint8")
    pinned = torch.zeros(size, dtype=torch.uint8).pin_memory()
    hold_ms = 60.0

    def fill(pattern, wait):
        torch.cuda.synchronize()
        T.hold(null, hold_ms)
        t0 = time.perf_counter()
        rc = rt.hipMemset(d.data_ptr(), pattern, size)
        if wait and rc == 0:
            rc = rt.hipStreamSynchronize(None)
        took = (time.perf_counter() - t0) * 1e3
        busy = T.pending(null)
        with torch.cuda.stream(side):
            pinned.copy_(d, non_blocking=True)
        side.synchronize()
        got = pinned.numpy().copy()
        torch.cuda.synchronize()
        print(f"stream-order: hipMemset of {size} bytes{' + a wait for the null stream' if wait else ''} behind a null-stream hold of {hold_ms:.0f} ms "
              f"took {took:.2f} ms; the null stream was {'still busy' if busy else 'idle'} at return; {int((got == pattern).sum())} of {size} bytes "
              "held the pattern")
        assert rc == 0
        return got

    fill(0x5A, wait=False)  # the raw call: observed, not relied on
    got = fill(0xA5, wait=True)
    assert (got == 0xA5).all(), "hipMemset and a wait for the null stream had not written the pattern at return"


@pytest.mark.parametrize("size", [4, 2048, 96 << 10])
def test_runtime_pageable_copy_has_taken_its_bytes_at_return(size):
    """What the table copies and symsync's n_in rely on: hipMemcpyAsync from pageable host memory onto a busy stream has taken the
    bytes when it returns, so the host may rewrite them at once. Whether the call drained the stream is printed for the notes: the
    rows of the stages that make such a copy assert it did not (their stream is still pending behind the call)."""
    import torch
    rt = T.hip_runtime()
    side = T.side_stream()
    first = np.random.default_rng(size).integers(0, 256, size).astype(np.uint8)
    src = first.copy()  # pageable
    d = zeros(size, "uint8")
    torch.cuda.synchronize()
    hold_ms = 60.0
    T.hold(side, hold_ms)
    t0 = time.perf_counter()
    rc = rt.hipMemcpyAsync(d.data_ptr(), src.ctypes.data, size, 1, side.cuda_stream)  # 1: hipMemcpyHostToDevice
    took = (time.perf_counter() - t0) * 1e3
    still = T.pending(side)
    src[:] = first ^ 0xFF  # rewritten the moment the call returns
    side.synchronize()
    torch.cuda.synchronize()
    got = host(d)
    print(f"stream-order: hipMemcpyAsync of {size} pageable bytes onto a stream held for {hold_ms:.0f} ms took {took:.2f} ms; the stream was "
          f"{'still pending' if still else 'DRAINED'} at return; {int((got == first).sum())} of {size} bytes are the ones passed")
    assert rc == 0
    assert (got == first).all(), "the copy read the host bytes after the call had returned"


@pytest.mark.parametrize("name", list(ROWS), ids=list(ROWS))
def test_pending_calls_equal_the_serialized_ones(name):
    """A (rows without a waiting entry) and B (rows with one): the row's calls behind a hold on a non-blocking stream"""
    want, host_ms = reference(name)
    hold_ms = T.hold_for(host_ms)
    print(f"stream-order: {name}: host side of the enqueues {host_ms:.3f} ms, hold {hold_ms:.0f} ms")
    got = run_held(get_row(name), T.side_stream(), hold_ms)
    if get_row(name).check is not None:
        get_row(name).check(got)
    same(got, want, f"{name}: behind a hold")


@pytest.mark.parametrize("name", ["bbframer", "bbdeheader", "pulse"])
def test_a_handle_created_while_the_null_stream_is_busy(name):
    """The fills of a constructor are work on the null stream, which a caller's non-blocking stream does not wait for: a handle created
    while the null stream is held must not return before its zeros are on the device (memset_done of csrc/device_stage.h) -- so the
    null stream is idle when the constructor returns --, and its first calls, made at once on a side stream, give the bits of the
    serialized pass, the state getters included. (A constructor that returned with its fill pending would have the zeros land on
    the state AFTER these calls. The de-header's and the framer's constructors make no other synchronous call that would hide it.)"""
    import torch
    r = get_row(name)
    want, _ = reference(name)
    side, null = T.side_stream(), T.null_stream()
    c = r.prep(None)  # (these rows' buffers do not depend on the handle)
    torch.cuda.synchronize()
    T.hold(null, 30.0)
    o = r.make()
    returned_early = T.pending(null)
    for _, f in r.calls:
        f(o, c, side.cuda_stream)
    side.synchronize()
    torch.cuda.synchronize()
    got = r.collect(o, c)
    close(o)
    assert not returned_early, f"{name}: the constructor returned while the null stream, and with it the fill of its state, was still pending"
    same(got, want, f"{name}: created while the null stream was busy")


@pytest.mark.parametrize("a,b", PAIRS, ids=[a for a, _ in PAIRS])
def test_two_handles_on_two_held_streams(a, b):
    """Two handles of one stage with different parameters, each on its own held stream, the enqueues interleaved; the holds end
    together, so the kernels of the two overlap. Each handle gives its own bits."""
    import torch
    ra, rb = get_row(a), get_row(b)
    (want_a, ms_a), (want_b, ms_b) = reference(a), reference(b)
    hold_ms = T.hold_for(ms_a + ms_b)
    sa, sb = T.side_stream(), T.side_stream()
    assert sa.cuda_stream != sb.cuda_stream
    oa, ob = ra.make(), rb.make()
    ca, cb = ra.prep(oa), rb.prep(ob)
    torch.cuda.synchronize()
    T.hold(sa, hold_ms)
    T.hold(sb, hold_ms)
    for i in range(max(len(ra.calls), len(rb.calls))):
        for r, o, c, s in ((ra, oa, ca, sa), (rb, ob, cb, sb)):
            if i < len(r.calls):
                r.calls[i][1](o, c, s.cuda_stream)
    still = T.pending(sa), T.pending(sb)
    sa.synchronize()
    sb.synchronize()
    torch.cuda.synchronize()
    assert all(still), f"a stream had drained behind the last enqueue: {still}, hold {hold_ms:.0f} ms"
    same(ra.collect(oa, ca), want_a, a)
    same(rb.collect(ob, cb), want_b, b)
    close(oa)
    close(ob)
