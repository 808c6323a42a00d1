"""Polyphase filter bank channelizer on the device (dvbs2_pfbch_*). The expected output is model (a) of tests/pfbch_model.py: every output
sample BIT FOR BIT (uint32 compare; a NaN equals a NaN) into sentinel-filled buffers whose pads and gaps must stay untouched, with zeros
of both signs and denormals planted in the input; the host's counter against Python integers after every call; the device against the
float64 model under the derived bound and against the device's down-converter; and a closed loop: two carriers on the channel grid, each
back through its own row and the receive stages of this library."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import ddc_model as DM
import fec_testlib as T
import loopback as L
import pfbch_model as PM
import pulse_model as PU
import test_ddc_gpu as DG  # the closed loop's receive side and constants; its capture is restated below for carriers on the grid
from dvbs2rx_amd import Agc, Awgn, Ddc, PfbChannelizer, PlSync, PulseShaper, Rotator, SymbolSync, awgn_sigma, capi, pfbch_tile, pulse_taps
from fec_testlib import PAD, SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def data(seed, n):
    x = PU.planted(np.random.default_rng(seed), n)
    x.setflags(write=False)
    return x


def same(got, want, what):
    """got: uint32 (n, 2) samples from the device; want: the model's complex64 row. The same bits; where the model has a NaN the device has
    one (the payload of a NaN that an operation creates is the processor's own)."""
    w = PM.bits(want).reshape(-1, 2)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    ok = (got == w) | (np.isnan(got.view(np.float32)) & np.isnan(w.view(np.float32)))
    if not ok.all():
        bad = np.nonzero(~ok.all(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {w.shape[0]} samples differ, the first at {bad[0]}: {got[bad[0]]} != {w[bad[0]]}")


class Expect:
    """what a handle must write and hold: model (a) with the history of every stream, the selection and the counter in Python integers"""

    def __init__(self, ch, taps, n_streams=1):
        self.ch, self.taps, self.M, self.D = ch, np.ascontiguousarray(taps, np.float32), ch.n_chan, ch.decim
        self.sel, self.n_streams = list(range(ch.n_chan)), n_streams
        self.reset(device_too=False)

    def reset(self, device_too=True):
        if device_too:
            self.ch.reset()
        self.hist, self.position = [None] * self.n_streams, 0

    def set_channels(self, sel):
        self.ch.set_channels(sel)
        self.sel = list(sel)
        assert self.ch.channels() == self.sel

    def work(self, xs):
        rows = []
        for s, x in enumerate(xs):
            y, self.hist[s] = PM.channelize32(self.taps, self.M, self.D, x, self.position, self.hist[s], self.sel)
            rows += list(y)
        self.position += xs[0].size
        return rows

    def state_is(self, what):
        assert self.ch.position() == self.position and self.ch.channels() == self.sel, what
        for n_in in (0, 1, min(97, self.ch.max_samples)):
            assert self.ch.produce(n_in) == PM.produce(self.position, self.D, n_in), what


def run_on_device(ch, xs, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the streams xs (complex64 vectors of one length n) through fec_testlib.run_strided: stream s lies at
    in_shift + s * in_stride complex elements of the input buffer, row i of stream s at out_shift + (s * n_sel + i) * out_stride of a
    sentinel buffer. Returns one uint32 (n_out, 2) array per row after checking the reported count against produce() before the call."""
    ns, n, n_sel = len(xs), xs[0].size, len(ch.channels())
    said = ch.produce(n)
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(said, 1) if out_stride is None else out_stride
    outs, n_out = T.run_strided(lambda a, o: ch.work_device(a, in_stride, n, ns, o, out_stride, stream()), xs, [said] * (ns * n_sel),
                                in_stride, out_stride, in_shift, out_shift)
    assert n_out == said == PM.produce(ch.position() - n, ch.decim, n)
    return outs


def call(e, xs, what, **where):
    got = run_on_device(e.ch, xs, **where)
    want = e.work(xs)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"{what}, row {i}")
    e.state_is(what)
    return got


# ------------------------------------------------------------------ 1. bit for bit over M, D, filter lengths and tile edges
def _cases():
    """A pruned product: every (M, D) pair of M in {2, 4, 8, 16 | 32, 64, 256} (16 and 32 are the two sides of the kernel's one switch,
    registers against LDS) with D in {M, M / 2, 1, 3, M - 1}, twice, the filter lengths {1, M - 1, M, M + 1, 2 M + 1, 4096} and the output
    counts {tile - 1, tile, tile + 1, 2 tile + 3} going round: 62 cases with every value of every axis. Two more for M = 128, the one
    build of the kernel (4 + 3 stages, its own segment length) that the axes leave out."""
    out, i = [], 0
    for M in (2, 4, 8, 16, 32, 64, 256):
        assert (M <= PM.REGISTER_MAX) == (M <= 16)
        for D in dict.fromkeys(d for d in (M, M // 2, 1, 3, M - 1) if 1 <= d <= M):
            for _ in range(2):
                ntaps = max((1, M - 1, M, M + 1, 2 * M + 1, 4096)[i % 6], 1)
                out.append((M, D, ntaps, (i + i // 6) % 4))
                i += 1
    out += [(128, 3, 2 * 128 + 1, 3), (128, 64, 4096, 1)]
    return out


def test_the_cases_keep_every_value_of_every_axis():
    cases = _cases()
    assert 55 <= len(cases) <= 65 and {c[3] for c in cases} == {0, 1, 2, 3}
    assert {(M, M % D == 0) for M, D, _, _ in cases} >= {(M, d) for M in (4, 8, 16, 32, 64, 256) for d in (True, False)} | {(2, True)}
    for M in (2, 4, 8, 16, 32, 64, 256):
        assert {D for m, D, _, _ in cases if m == M} == {d for d in (M, M // 2, 1, 3, M - 1) if 1 <= d <= M}
    kinds = {("1", "M-1", "M", "M+1", "2M+1", "4096")[j] for M, _, ntaps, _ in cases for j, v in enumerate((1, M - 1, M, M + 1, 2 * M + 1, 4096)) if ntaps == v}
    assert len(kinds) == 6


@pytest.mark.parametrize("M,D,ntaps,which", _cases())
def test_bit_for_bit_at_the_tile_edges(M, D, ntaps, which):
    """From a reset handle the shortest call that writes tile - 1, tile, tile + 1 or 2 tile + 3 outputs, followed by calls of 0, 1, D - 1
    and 40 samples that go on from its history (shorter than the history: old history and input both enter the new one) and from
    positions that are no multiples of D or M; then the same short calls on a handle that has nothing but zeros behind it."""
    rng = np.random.default_rng(100000 * M + 1000 * D + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    tile = pfbch_tile(M, D, ntaps)
    target = (tile - 1, tile, tile + 1, 2 * tile + 3)[which]
    n_in = (target - 1) * D + 1  # the first output uses the first sample, the last output the last
    ch = PfbChannelizer(M, D, taps, max_samples=max(n_in, 40))
    assert (ch.n_chan, ch.decim, ch.ntaps, ch.history, ch.delay_num, ch.tile) == (M, D, ntaps, ntaps - 1, ntaps - 1, tile) and tile == PM.tile(M, D, ntaps)
    e = Expect(ch, taps)
    assert PM.produce(0, D, n_in) == target and PM.produce(0, D, n_in - 1) == target - 1
    what = f"M {M} D {D} ntaps {ntaps}"
    call(e, [data(M * 10000 + D * 100 + n_in % 9973, n_in)], f"{what}: {target} outputs")
    for more in (0, 1, D - 1, 40):
        call(e, [data(7 + more, max(more, 1))[:more]], f"{what}: {more} samples behind {target} outputs")
    e.reset()
    for first in (0, 1, D - 1):
        call(e, [data(17 + first, max(first, 1))[:first]], f"{what}: {first} samples from a reset handle")
    ch.close()


# ------------------------------------------------------------------ 2. special values
@pytest.mark.parametrize("M,D,ntaps", [(8, 3, 11), (64, 32, 130)])
def test_special_values(M, D, ntaps):
    """inf, NaN, denormals and -0.0 in the input come out as the model's own float32 operations give them: a tap that a branch does not
    have contributes nothing (0 * inf would be a NaN), non-finite values spread through the transform as IEEE says."""
    taps = np.random.default_rng(M).normal(size=ntaps).astype(np.float32)
    x = np.array(data(900 + M, 40 * D + ntaps))
    x[5 * D + 1] = np.complex64(complex(np.inf, 1.0))
    x[17 * D] = np.complex64(complex(2.0, np.nan))
    x[25 * D + 2] = np.complex64(complex(-np.inf, -0.0))
    x[30 * D:31 * D + 3] = np.complex64(complex(-1e-41, 1e-41))
    ch = PfbChannelizer(M, D, taps, max_samples=x.size)
    e = Expect(ch, taps)
    want = e.work([x])
    e.reset(device_too=False)
    got = call(e, [x], f"special values, M {M}")
    g = np.stack(got).view(np.float32)
    assert np.isnan(g).any() and np.isinf(g).any() and np.isfinite(g).all(axis=(0, 2)).sum() >= 20
    assert np.isfinite(np.stack(want)).all(axis=0).sum() == np.isfinite(g).all(axis=(0, 2)).sum()
    ch.close()


# ------------------------------------------------------------------ 3. placement
@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M", [8, 32])
def test_placement_strides_streams_and_selection(M, in_shift, out_shift):
    """Buffers displaced by one complex element are 8-byte but not 16-byte aligned; strides wider than needed; 3 streams; 3 of the
    channels in scrambled order: rows that are not selected do not exist, and everything between and behind the rows stays sentinel
    (run_strided checks it)."""
    D, ntaps = 3, 2 * M + 3
    taps = np.random.default_rng(5).normal(size=ntaps).astype(np.float32)
    n_in = (pfbch_tile(M, D, ntaps) + 9) * D + 1
    ch = PfbChannelizer(M, D, taps, max_streams=3, max_samples=n_in)
    e = Expect(ch, taps, n_streams=3)
    e.set_channels([5, 0, 3])
    xs = [data(60 + s, n_in) for s in range(3)]
    got = call(e, xs, f"shifts {in_shift} {out_shift}", in_stride=n_in + 3 + (in_shift ^ 1), out_stride=ch.produce(n_in) + 5 + out_shift,
               in_shift=in_shift, out_shift=out_shift)
    assert len(got) == 9 and not np.array_equal(got[0], got[3])
    call(e, [x[:50] for x in xs[:2]], "two of three streams", in_stride=64)  # (the third stream's history stays; it is not used again)
    ch.close()


# ------------------------------------------------------------------ 4. cuts
@pytest.mark.parametrize("M,D,ntaps", [(8, 3, 40), (16, 8, 5), (8, 4, 1), (32, 12, 77), (256, 128, 4096)])
def test_cuts_give_the_bits_of_one_call(M, D, ntaps):
    """A stream in one call equals the same stream in cuts -- 3 M + 1, 0, 1, D - 1, 5, random ones and the rest -- with the selection
    changed between cuts (the rows are compared channel by channel) and, after a reset in the middle, once more from the start."""
    rng = np.random.default_rng(M + D + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    tile = pfbch_tile(M, D, ntaps)
    n = (2 * tile + 5) * D + D // 2 + 3 * M
    x = data(40 + M, n)
    ch = PfbChannelizer(M, D, taps, max_samples=n)
    e = Expect(ch, taps)
    whole = call(e, [x], "one call")
    for round_ in range(2):
        e.reset()  # (the second round: a reset in the middle of a stream of cuts gives the start again)
        cuts = [3 * M + 1, 0, 1, D - 1, 5] + [int(c) for c in rng.integers(1, tile * D // 2 + 2, 3)]
        assert sum(cuts) < n
        cuts.append(n - sum(cuts))
        parts, pos = [[] for _ in range(M)], 0
        for i, c in enumerate(cuts):
            sel = list(range(M)) if i % 3 == 0 else [int(v) for v in rng.permutation(M)[:max(1, M // 2)]]
            e.set_channels(sel)
            got = call(e, [x[pos:pos + c]], f"cut of {c} at {pos}")
            for row, chan in zip(got, sel):
                parts[chan].append((pos, row))
            pos += c
            if round_ == 0 and i == 4:
                break
        if round_ == 0:
            continue
        assert pos == n
        for chan in range(M):  # every piece a channel was selected for equals the one call's samples at its place
            for start, row in parts[chan]:
                o = PM.produce(0, D, start)
                assert np.array_equal(row, whole[chan][o:o + row.shape[0]]), (chan, start)
    ch.close()


def test_host_entry_equals_the_device_entry():
    M, D, taps = 8, 4, pulse_taps(16, 0.35, 4, 0.0, 1.0)
    a, b = PfbChannelizer(M, D, taps, max_streams=2, max_samples=3000), PfbChannelizer(M, D, taps, max_streams=2, max_samples=3000)
    for ch in (a, b):
        ch.set_channels([6, 1, 2])
    for n in (3000, 3, 0, 1, 50):
        xs = np.stack([data(70 + n, max(n, 1))[:n], data(71 + n, max(n, 1))[:n]])
        got = a.work(xs)
        assert got.dtype == np.complex64 and got.shape == (2, 3, PM.produce(b.position(), D, n))
        if n:
            dev = run_on_device(b, [xs[0], xs[1]])
            for s in range(2):
                for i in range(3):
                    assert np.array_equal(dev[3 * s + i], PM.bits(got[s, i]).reshape(-1, 2)), (n, s, i)
        else:
            b.work_device(0, 0, 0, 2, 0, 0, stream())
        assert a.position() == b.position()
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. accuracy
@pytest.mark.parametrize("M,D,ntaps", [(8, 4, 65), (16, 16, 129), (64, 32, 513), (256, 128, 1025)])
def test_accuracy_against_the_float64_model(M, D, ntaps):
    """|device - exact| <= sqrt(2) gamma_q S (1 + B) + B ||w||_2 per output (tests/pfbch_model.py (c), notes/pfbch.md has the derivation
    and the worst ratios measured: 0.03-0.06 on these shapes)."""
    rng = np.random.default_rng(99 + M)
    taps = (rng.normal(size=ntaps) / math.sqrt(ntaps)).astype(np.float32)
    x = (rng.normal(size=60 * D + ntaps) + 1j * rng.normal(size=60 * D + ntaps)).astype(np.complex64)
    ch = PfbChannelizer(M, D, taps, max_samples=x.size)
    got = np.stack(run_on_device(ch, [x])).view(np.float32).astype(np.float64)
    got = got[..., 0] + 1j * got[..., 1]
    exact, S, w_norm = PM.channelize64(taps, M, D, x)
    err = np.abs(got - exact)
    ratio = float((err / PM.bound(M, ntaps, S, w_norm)[None, :]).max())
    print(f"accuracy M {M} D {D} ntaps {ntaps}: worst error / bound {ratio:.4f}, worst error {err.max():.3e}, output rms {np.sqrt(np.mean(np.abs(exact) ** 2)):.3f}")
    assert ratio <= 1.0
    ch.close()


def test_every_channel_against_the_device_ddc():
    """M 8, D 4, 65 designed taps: channel c against the device's down-converter with phase_inc = -2 pi c / M on the same input, within
    the sum of the two stages' bounds."""
    M, D, ntaps = 8, 4, 65
    k = np.arange(ntaps) - (ntaps - 1) / 2
    taps = (np.sinc(k / M) * np.hamming(ntaps) / M).astype(np.float32)
    rng = np.random.default_rng(3)
    x = (rng.normal(size=4000) + 1j * rng.normal(size=4000)).astype(np.complex64)
    ch = PfbChannelizer(M, D, taps, max_samples=x.size)
    dd = Ddc(D, taps, max_channels=M, max_samples=x.size)
    for c in range(M):
        dd.set_channel(c, -2.0 * np.pi * c / M)
    mine = np.stack(run_on_device(ch, [x])).view(np.float32).astype(np.float64)
    theirs = np.stack(DG.run_on_device(dd, [x], M)).view(np.float32).astype(np.float64)
    mine, theirs = mine[..., 0] + 1j * mine[..., 1], theirs[..., 0] + 1j * theirs[..., 1]
    _, S, w_norm = PM.channelize64(taps, M, D, x)
    own = PM.bound(M, ntaps, S, w_norm)
    gamma = ntaps * DM.U / (1.0 - ntaps * DM.U)
    worst = 0.0
    for c in range(M):
        _, mix_bound = DM.ddc64(taps, D, x, -2.0 * np.pi * c / M)
        ratio = float((np.abs(mine[c] - theirs[c]) / (own + math.sqrt(2.0) * (mix_bound + gamma * S))).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0 and np.abs(theirs[c]).max() > 1000 * np.abs(mine[c] - theirs[c]).max(), (c, ratio)
    print(f"against the device's down-converter: worst difference / bound {worst:.4f}")
    dd.close()
    ch.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_everything_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    good = np.ones(21, np.float32)
    gp = good.ctypes.data
    # creation (every argument refusal without a device: tests/test_pfbch_host.py)
    refused(capi.EINVAL, "n_chan must be a power of two in 2..256", lib.dvbs2_pfbch_create, C.byref(h), 6, 2, gp, 21, 1, 16, 0)
    refused(capi.EINVAL, "decim must be in 1..n_chan", lib.dvbs2_pfbch_create, C.byref(h), 8, 9, gp, 21, 1, 16, 0)
    refused(capi.EINVAL, "ntaps must be in 1..4096", lib.dvbs2_pfbch_create, C.byref(h), 8, 4, gp, 4097, 1, 16, 0)
    refused(capi.EINVAL, "null handle pointer", lib.dvbs2_pfbch_create, None, 8, 4, gp, 21, 1, 16, 0)
    assert not h
    assert lib.dvbs2_pfbch_create(C.byref(h), 8, 4, gp, 21, 1, 16, 99) < 0 and not h  # no such device

    M, D, n = 8, 4, 100
    taps = pulse_taps(8, 0.2, 2, 0.0, 1.0)
    ch = PfbChannelizer(M, D, taps, max_streams=2, max_samples=n)
    e = Expect(ch, taps, n_streams=2)
    e.set_channels([6, 1, 3])
    first, second = [data(80 + s, n) for s in range(2)], [data(90 + s, n) for s in range(2)]
    call(e, [x[:n - 1] for x in first], "before the refusals")  # (99 samples: the counter is no multiple of D)
    n_out = ch.produce(n)
    assert n_out == PM.produce(n - 1, D, n) == 25
    d_in = torch.from_numpy(np.concatenate(second).view(np.float32)).cuda()
    d_out = sentinel(2 * (6 * n_out + PAD))
    st = stream()
    a, o = d_in.data_ptr(), d_out.data_ptr()
    count = C.c_int64(-7)
    c = C.byref(count)
    entry = lib.dvbs2_pfbch_process_device
    refused(capi.ESIZE, "n_in exceeds max_samples", entry, ch._h, a, n, n + 1, 2, o, n_out, c, st)
    refused(capi.ESIZE, "n_streams exceeds max_streams", entry, ch._h, a, n, n, 3, o, n_out, c, st)
    refused(capi.EINVAL, "n_in is negative", entry, ch._h, a, n, -1, 2, o, n_out, c, st)
    refused(capi.EINVAL, "n_streams is negative", entry, ch._h, a, n, n, -1, o, n_out, c, st)
    refused(capi.EINVAL, "in is null", entry, ch._h, None, n, n, 2, o, n_out, c, st)
    refused(capi.EINVAL, "out is null", entry, ch._h, a, n, n, 2, None, n_out, c, st)
    refused(capi.EINVAL, "in and out must not be the same buffer", entry, ch._h, a, n, n, 2, a, n_out, c, st)
    refused(capi.EINVAL, "in_stride is below n_in", entry, ch._h, a, n - 1, n, 2, o, n_out, c, st)
    refused(capi.EINVAL, "out_stride is below n_out", entry, ch._h, a, n, n, 2, o, n_out - 1, c, st)  # before any launch
    refused(capi.EINVAL, "out_stride is below n_out", entry, ch._h, a, n, n, 1, o, n_out - 1, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, ch._h, a + 4, n, n, 2, o, n_out, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, ch._h, a, n, n, 2, o + 4, n_out, c, st)
    assert count.value == -7
    bad = np.array([5, 2, 5, 8, -1], np.int32)
    refused(capi.EINVAL, "n_sel must be in 1..n_chan", lib.dvbs2_pfbch_set_channels, ch._h, bad.ctypes.data, 0)
    refused(capi.EINVAL, "n_sel must be in 1..n_chan", lib.dvbs2_pfbch_set_channels, ch._h, bad.ctypes.data, 9)
    refused(capi.EINVAL, "null list", lib.dvbs2_pfbch_set_channels, ch._h, None, 2)
    refused(capi.EINVAL, "list[2] repeats a channel", lib.dvbs2_pfbch_set_channels, ch._h, bad.ctypes.data, 3)
    refused(capi.EINVAL, "list[1] is not a channel", lib.dvbs2_pfbch_set_channels, ch._h, bad[2:].ctypes.data, 2)
    refused(capi.EINVAL, "list[0] is not a channel", lib.dvbs2_pfbch_set_channels, ch._h, bad[4:].ctypes.data, 1)
    refused(capi.EINVAL, "counter is null", lib.dvbs2_pfbch_position, ch._h, None)
    assert entry(ch._h, None, 0, 0, 2, None, 0, c, st) == capi.OK  # n_in == 0: a successful call that does nothing and reports 0
    assert count.value == 0
    e.state_is("behind the refusals")
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = np.stack(second), np.zeros((6, n_out), np.complex64)
    count = C.c_int64(-7)
    c = C.byref(count)
    host = lib.dvbs2_pfbch_process
    hi, ho = host_in.ctypes.data, host_out.ctypes.data
    refused(capi.ESIZE, "n_in exceeds max_samples", host, ch._h, hi, n, n + 1, 2, ho, n_out, c)
    refused(capi.EINVAL, "n_in is negative", host, ch._h, hi, n, -1, 2, ho, n_out, c)
    refused(capi.EINVAL, "in is null", host, ch._h, None, n, n, 2, ho, n_out, c)
    refused(capi.EINVAL, "out is null", host, ch._h, hi, n, n, 2, None, n_out, c)
    refused(capi.EINVAL, "in_stride is below n_in", host, ch._h, hi, n - 1, n, 2, ho, n_out, c)
    refused(capi.EINVAL, "out_stride is below n_out", host, ch._h, hi, n, n, 2, ho, n_out - 1, c)
    assert (host_out == 0).all() and count.value == -7
    # no refusal touched a history, the counter or the selection: both streams go on from where the good call left them
    e.state_is("behind the host entry's refusals")
    call(e, second, "behind the refusals")
    # a call without streams only advances the counter
    assert ch.work_device(d_in.data_ptr(), n, 10, 0, 0, 0, st) == PM.produce(e.position, D, 10)
    e.position += 10
    e.state_is("behind a call without streams")
    ch.close()


# ------------------------------------------------------------------ 7. closed loop: two carriers on the channel grid
CHANNELS = (1, 6)  # of M = 8: +1/8 and +6/8 (that is -2/8) cycles per sample, 3 symbol rates apart at 8 samples per symbol


@functools.lru_cache(maxsize=None)
def capture():
    """test_ddc_gpu.capture with the carriers on the grid: two carriers of short QPSK 1/4 frames with different payloads, each shaped at 8
    samples per symbol with roll-off 0.2 (taps scaled so that the symbols behind the channel filter have unit amplitude), moved to
    +2 pi 1/8 and +2 pi 6/8 radians per sample and added; noise at Es/N0 = 10 dB for the power of one carrier; all of it scaled by 1/37.
    Returns (the encoders' inputs [2], the samples on the device, their number, symbols per carrier)."""
    import torch
    st = stream()
    sps = DG.SPS
    rx = pulse_taps(sps, DG.ROLLOFF, DG.RRC_DELAY, 0.0, 1.0)
    tx = pulse_taps(sps, DG.ROLLOFF, DG.RRC_DELAY).astype(np.float64)
    tx = (tx / np.convolve(tx, rx.astype(np.float64))[2 * sps * DG.RRC_DELAY]).astype(np.float32)
    d_sum, sent, power = None, [], []
    for k, chan in enumerate(CHANNELS):
        sent_k, d_x, n, n_all, _ = L.transmit_symbols(DG.SEQ, DG.ND, L.GOLD, DG.LEAD, seed=3000 + k, flush=256)
        sent.append(sent_k)
        ns = n_all * sps
        ps = PulseShaper(sps, taps=tx, max_symbols=n_all)
        d_y = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
        ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), ns, st)
        power.append(float((d_y[:n * sps] ** 2).sum(dim=1).mean().item()))
        rot = Rotator(2.0 * np.pi * chan / 8)
        rot.work_device(d_y.data_ptr(), ns, d_y.data_ptr(), st)
        if d_sum is None:
            d_sum = torch.zeros_like(d_y)
        d_sum += d_y
        torch.cuda.synchronize()
        rot.close()
        ps.close()
    assert abs(power[0] / power[1] - 1) < 0.05
    noise = Awgn(seed=77, sigma=awgn_sigma(DG.ES_N0_DB, es=power[0], sps=sps), max_samples=ns)
    noise.work_device(d_sum.data_ptr(), ns, ns, 1, d_sum.data_ptr(), ns, first_index=0, stream=st)
    d_sum *= DG.SCALE
    torch.cuda.synchronize()
    noise.close()
    return sent, d_sum, ns, n_all


def channelize(sel):
    import torch
    sent, d_wide, ns, n_all = capture()
    assert (DG.SPS, DG.ROLLOFF, DG.RRC_DELAY, DG.ES_N0_DB, DG.SCALE) == (8, 0.2, 5, 10.0, 1.0 / 37.0)
    ch = PfbChannelizer(8, 4, pulse_taps(8, 0.2, 5, 0, 1), max_samples=ns)
    ch.set_channels(sel)
    n_out = ch.produce(ns)
    assert n_out == ns // 4  # 2 samples per symbol
    d_rows = torch.zeros((len(sel), n_out, 2), dtype=torch.float32, device="cuda")
    assert ch.work_device(d_wide.data_ptr(), ns, ns, 1, d_rows.data_ptr(), n_out, stream()) == n_out
    torch.cuda.synchronize()
    ch.close()
    return sent, d_rows, n_out, n_all


def test_closed_loop_each_row_returns_its_own_carrier():
    """set_channels([6, 1]): row 0 returns the bytes of the carrier in channel 6, row 1 those of the carrier in channel 1, neither the
    other's: the sign of the transform and the order of the selection are pinned."""
    sent, d_rows, n_out, n_all = channelize([6, 1])
    for row, chan in enumerate((6, 1)):
        carrier = CHANNELS.index(chan)
        msg, data_index = DG.receive(d_rows[row], n_out, n_all, f"row {row} (channel {chan})")
        assert np.array_equal(msg, sent[carrier][data_index]), (row, chan)  # the encoder's input bytes
        assert not np.array_equal(msg, sent[carrier ^ 1][data_index])


def test_closed_loop_the_mirror_channels_hold_no_carrier():
    """set_channels([7, 2]), the mirror images of channels 1 and 6: behind the same AGC and timing recovery the frame search does not
    reach PLSYNC_LOCKED on either row."""
    import torch
    _, d_rows, n_out, _ = channelize([7, 2])
    st = stream()
    for row in range(2):
        d_y = d_rows[row]
        reference = float(torch.linalg.vector_norm(d_y[:2 * DG.LEAD], dim=1).mean().item()) / DG.SCALE
        agc = Agc(rate=0.05, reference=reference, gain=1.0, max_gain=65536.0, max_samples=n_out)
        d_g = torch.zeros_like(d_y)
        d_gain = torch.zeros(n_out, dtype=torch.float32, device="cuda")
        agc.work_device(d_y.data_ptr(), n_out, n_out, 1, d_g.data_ptr(), n_out, d_gain.data_ptr(), n_out, st)
        ss = SymbolSync(sps=2, loop_bw=0.01, damping=1.0, rolloff=DG.ROLLOFF, interp_method=SymbolSync.CUBIC, max_samples=n_out)
        d_sym = torch.zeros(2 * n_out, dtype=torch.float32, device="cuda")
        ss.work_device(d_g.data_ptr(), n_out, [n_out], d_sym.data_ptr(), n_out, n_out, 0, 0, st)
        n_sym, _, status = ss.finish()
        nsym = int(n_sym[0])
        ss.close()
        agc.close()
        assert status[0] == 0 and nsym > n_out // 4
        sync = PlSync(plsc=-1, max_symbols=max(nsym, PlSync.MIN_SYMBOLS), max_frames=64)
        d_rec = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
        sync.work_device(d_sym.data_ptr(), nsym, d_rec.data_ptr(), st)
        nf, _, state = sync.finish()
        sync.close()
        print(f"mirror row {row}: {nsym} symbols, {nf} frame records, state {state}")
        assert state != capi.PLSYNC_LOCKED
