"""Polyphase synthesis filter bank on the device (dvbs2_pfbsyn_*). The expected output is model (a) of tests/pfbsyn_model.py: every output
sample BIT FOR BIT (uint32 compare; a NaN equals a NaN) into sentinel-filled buffers whose pads and gaps must stay untouched, with zeros
of both signs and denormals planted in the input; the host's counter against Python integers after every call; the device against the
float64 model under the derived bound and against the device route the stage replaces (pulse shaper, rotator and sum per row); and a
closed loop: the PLFRAME symbols of two carriers through the synthesizer, noise, the channelizer and the receive stages of this library."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import pfbsyn_model as SY
import plcoarse_model as PC
import pulse_model as PU
import test_ddc_gpu as DG  # the closed loop's receive side and constants
from dvbs2rx_amd import Agc, Awgn, PfbChannelizer, PfbSynthesizer, PlSync, PulseShaper, Rotator, SymbolSync, awgn_sigma, capi, pfbsyn_tile, pulse_taps
from fec_testlib import PAD, SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def data(seed, n_rows, n):
    """[n_rows, n] complex64 with zeros of both signs and denormals planted"""
    x = PU.planted(np.random.default_rng(seed), max(n_rows * n, 16))[:n_rows * n].reshape(n_rows, n).copy()
    x.setflags(write=False)
    return x


def same(got, want, what):
    """got: uint32 (n, 2) samples from the device; want: the model's complex64 vector. The same bits; where the model has a NaN the device
    has one (the payload of a NaN that an operation creates is the processor's own)."""
    w = SY.bits(want).reshape(-1, 2)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    ok = (got == w) | (np.isnan(got.view(np.float32)) & np.isnan(w.view(np.float32)))
    if not ok.all():
        bad = np.nonzero(~ok.all(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {w.shape[0]} samples differ, the first at {bad[0]}: {got[bad[0]]} != {w[bad[0]]}")


class Expect:
    """what a handle must write and hold: model (a) with the tail of every stream, the selection and the counter in Python integers"""

    def __init__(self, sy, taps, n_streams=1):
        self.sy, self.taps, self.M, self.L = sy, np.ascontiguousarray(taps, np.float32), sy.n_chan, sy.interp
        self.sel, self.n_streams = list(range(sy.n_chan)), n_streams
        self.reset(device_too=False)

    def reset(self, device_too=True):
        if device_too:
            self.sy.reset()
        self.tail, self.position = [None] * self.n_streams, 0

    def set_channels(self, sel):
        self.sy.set_channels(sel)
        self.sel = list(sel)
        assert self.sy.channels() == self.sel

    def work(self, xs):
        out = []
        for s, x in enumerate(xs):
            y, self.tail[s] = SY.synth32(self.taps, self.M, self.L, x, self.position, self.tail[s], self.sel)
            out.append(y)
        self.position += xs[0].shape[1]
        return out

    def state_is(self, what):
        assert self.sy.position() == self.position and self.sy.channels() == self.sel, what


def run_on_device(sy, xs, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the streams xs (complex64 [n_sel, n] each) through fec_testlib.run_strided: row i of stream s lies at
    in_shift + (s * n_sel + i) * in_stride complex elements of the input buffer, stream s writes at out_shift + s * out_stride of a
    sentinel buffer. Returns one uint32 (n * L, 2) array per stream after checking the reported count."""
    ns, n_sel, n = len(xs), len(sy.channels()), xs[0].shape[1]
    assert all(x.shape == (n_sel, n) for x in xs)
    said = sy.produce(n)
    assert said == n * sy.interp
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(said, 1) if out_stride is None else out_stride
    flat = [np.ascontiguousarray(row) for x in xs for row in x]
    outs, n_out = T.run_strided(lambda a, o: sy.work_device(a, in_stride, n, ns, o, out_stride, stream()), flat, [said] * ns,
                                in_stride, out_stride, in_shift, out_shift)
    assert n_out == said
    return outs


def call(e, xs, what, **where):
    before = e.position
    got = run_on_device(e.sy, xs, **where)
    want = e.work(xs)
    assert len(got) == len(want) and e.position == before + xs[0].shape[1]
    for s, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"{what}, stream {s}")
    e.state_is(what)
    return got


def largest(M, L):
    """the longest filter that creation accepts at (M, L)"""
    return min(SY.MAX_TAPS, (SY.MAX_PRODUCT // M) * L)


# ------------------------------------------------------------------ 1. bit for bit over M, L, filter lengths and tile edges
def _cases():
    """A pruned product: every (M, L) pair of M in {2, 4, 8, 16 | 32, 64, 256} (16 and 32 are the two sides of the kernel's one switch,
    a lane's registers against two passes through LDS) with L in {M, M / 2, 1, 3, M - 1}, twice, the filter lengths {1, L - 1, L, L + 1,
    2 L + 1, the largest legal} and the instant counts {tile - 1, tile, tile + 1, 2 tile + 3} going round. Two more for M = 128, the one
    build of the kernel (4 + 3 stages, its own segment length) that the axes leave out."""
    out, i = [], 0
    for M in (2, 4, 8, 16, 32, 64, 256):
        assert (M <= SY.REGISTER_MAX) == (M <= 16)
        for Li in dict.fromkeys(d for d in (M, M // 2, 1, 3, M - 1) if 1 <= d <= M):
            for _ in range(2):
                ntaps = max((1, Li - 1, Li, Li + 1, 2 * Li + 1, largest(M, Li))[i % 6], 1)
                out.append((M, Li, min(ntaps, largest(M, Li)), (i + i // 6) % 4))
                i += 1
    out += [(128, 3, 2 * 3 + 1, 3), (128, 64, 4096, 1)]
    return out


def test_the_cases_keep_every_value_of_every_axis():
    cases = _cases()
    assert 55 <= len(cases) <= 65 and {c[3] for c in cases} == {0, 1, 2, 3}
    assert all(SY.legal(M, Li, ntaps) for M, Li, ntaps, _ in cases)
    assert {(M, M % Li == 0) for M, Li, _, _ in cases} >= {(M, d) for M in (4, 8, 16, 32, 64, 256) for d in (True, False)} | {(2, True)}
    for M in (2, 4, 8, 16, 32, 64, 256):
        assert {Li for m, Li, _, _ in cases if m == M} == {d for d in (M, M // 2, 1, 3, M - 1) if 1 <= d <= M}
    names = ("1", "L-1", "L", "L+1", "2L+1", "largest")
    kinds = {names[j] for M, Li, ntaps, _ in cases for j, v in enumerate((1, Li - 1, Li, Li + 1, 2 * Li + 1, largest(M, Li))) if ntaps == v}
    assert len(kinds) == 6
    assert any(ntaps == largest(M, Li) and ntaps > 2 * Li + 1 for M, Li, ntaps, _ in cases)
    # both tile rules, a tail longer than a tile's outputs, no tail at all
    assert {pfbsyn_tile(M, Li, ntaps) + -(-ntaps // Li) - 1 > SY.SPAN // SY.seg_len(M) for M, Li, ntaps, _ in cases} == {True, False}
    assert any(ntaps <= Li for _, Li, ntaps, _ in cases) and any(ntaps - Li > pfbsyn_tile(M, Li, ntaps) * Li for M, Li, ntaps, _ in cases)


@pytest.mark.parametrize("M,Li,ntaps,which", _cases())
def test_bit_for_bit_at_the_tile_edges(M, Li, ntaps, which):
    """From a reset handle a call of tile - 1, tile, tile + 1 or 2 tile + 3 instants, followed by calls of 0, 1, 2 and 40 instants that
    go on from its tail (shorter than the tail where the filter is long: the old tail and the call's instants both enter the new one)
    and from counters whose outputs start off the multiples of M; then the same short calls on a handle after a reset."""
    rng = np.random.default_rng(100000 * M + 1000 * Li + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    tile = pfbsyn_tile(M, Li, ntaps)
    n_in = (tile - 1, tile, tile + 1, 2 * tile + 3)[which]
    sy = PfbSynthesizer(M, Li, taps, max_samples=max(n_in, 40))
    assert (sy.n_chan, sy.interp, sy.ntaps, sy.tail, sy.delay_num, sy.tile) == (M, Li, ntaps, max(ntaps - Li, 0), ntaps - 1, tile) and tile == SY.tile(M, Li, ntaps)
    e = Expect(sy, taps)
    what = f"M {M} L {Li} ntaps {ntaps}"
    call(e, [data(M * 10000 + Li * 100 + n_in % 9973, M, n_in)], f"{what}: {n_in} instants")
    for more in (0, 1, 2, 40):
        call(e, [data(7 + more, M, more)], f"{what}: {more} instants behind {n_in}")
    e.reset()
    for first in (0, 1, 2):
        call(e, [data(17 + first, M, first)], f"{what}: {first} instants from a reset handle")
    sy.close()


# ------------------------------------------------------------------ 2. special values
@pytest.mark.parametrize("M,Li,ntaps", [(8, 3, 11), (64, 32, 130)])
def test_special_values(M, Li, ntaps):
    """inf, NaN, denormals and -0.0 in the input come out as the model's own float32 operations give them: an instant that does not
    exist contributes nothing (0 * inf would be a NaN), non-finite values spread through the transform as IEEE says and reach exactly the
    outputs whose taps meet their instants."""
    taps = np.random.default_rng(M).normal(size=ntaps).astype(np.float32)
    x = np.array(data(900 + M, M, 60))
    x[0, 0] = np.complex64(complex(np.inf, 1.0))  # the first instant: the instants before it are skipped, not multiplied
    x[M // 2, 17] = np.complex64(complex(2.0, np.nan))
    x[M - 1, 25] = np.complex64(complex(-np.inf, -0.0))
    x[:, 40:42] = np.complex64(complex(-1e-41, 1e-41))
    sy = PfbSynthesizer(M, Li, taps, max_samples=60)
    e = Expect(sy, taps)
    got = call(e, [x], f"special values, M {M}")[0].view(np.float32)
    finite = np.isfinite(got).all(axis=1)
    n = np.arange(60 * Li)
    reached = np.zeros(60 * Li, bool)
    for k in (0, 17, 25):
        reached |= (n >= k * Li) & (n < k * Li + ntaps)
    assert np.isnan(got).any() and np.isinf(got).any() and not (~finite & ~reached).any() and (~finite).sum() >= 2 * ntaps and finite.sum() >= 20
    call(e, [np.array(data(5, M, 3))], "behind them")  # the tail carries what is left of them
    sy.close()


# ------------------------------------------------------------------ 3. placement
@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M", [8, 32])
def test_placement_strides_streams_and_selection(M, in_shift, out_shift):
    """Buffers displaced by one complex element are 8-byte but not 16-byte aligned; strides wider than needed; 3 streams; 3 of the
    channels fed in scrambled order: everything between and behind the n_in * L outputs of every stream stays sentinel and the input
    is not written (run_strided checks both)."""
    Li, ntaps = 3, 2 * M + 3
    taps = np.random.default_rng(5).normal(size=ntaps).astype(np.float32)
    n_in = pfbsyn_tile(M, Li, ntaps) + 9
    sy = PfbSynthesizer(M, Li, taps, max_streams=3, max_samples=n_in)
    e = Expect(sy, taps, n_streams=3)
    e.set_channels([5, 0, 3])
    xs = [data(60 + s, 3, n_in) for s in range(3)]
    got = call(e, xs, f"shifts {in_shift} {out_shift}", in_stride=n_in + 3 + (in_shift ^ 1), out_stride=n_in * Li + 5 + out_shift,
               in_shift=in_shift, out_shift=out_shift)
    assert len(got) == 3 and not np.array_equal(got[0], got[1])
    call(e, [x[:, :50] for x in xs[:2]], "two of three streams", in_stride=64)
    call(e, [x[:, 50:70] for x in xs], "all three again: the third goes on from the tail the first call left", in_stride=32)
    sy.close()


# ------------------------------------------------------------------ 4. cuts
@pytest.mark.parametrize("M,Li,ntaps", [(8, 3, 40), (16, 8, 5), (8, 4, 1), (32, 12, 77), (256, 128, 4096)])
def test_cuts_give_the_bits_of_one_call(M, Li, ntaps):
    """A stream in one call equals the same stream in cuts -- 3, 0, 1, 2, 40, random ones and the rest -- with the selection changed
    between cuts (the one call is fed the rows of every cut at their channels and zeros elsewhere) and, after a reset in the middle,
    once more from the start."""
    rng = np.random.default_rng(M + Li + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    tile = pfbsyn_tile(M, Li, ntaps)
    n = 2 * tile + 60
    cuts = [3, 0, 1, 2, 40] + [int(c) for c in rng.integers(1, tile // 2 + 2, 3)]
    assert sum(cuts) < n
    cuts.append(n - sum(cuts))
    sels = [list(range(M)) if i % 3 == 0 else [int(v) for v in rng.permutation(M)[:max(1, M // 2)]] for i in range(len(cuts))]
    whole_in, pieces, pos = np.zeros((M, n), np.complex64), [], 0
    for c, sel in zip(cuts, sels):
        x = np.array(data(40 + M + pos, len(sel), c))
        whole_in[sel, pos:pos + c] = x
        pieces.append(x)
        pos += c
    sy = PfbSynthesizer(M, Li, taps, max_samples=n)
    e = Expect(sy, taps)
    whole = call(e, [whole_in], "one call")[0]
    for round_ in range(2):
        e.reset()  # (the second round: a reset in the middle of a stream of cuts gives the start again)
        parts = []
        for i, (x, sel) in enumerate(zip(pieces, sels)):
            e.set_channels(sel)
            parts.append(call(e, [x], f"cut {i} of {x.shape[1]}")[0])
            if round_ == 0 and i == 4:
                break
        if round_:
            assert np.array_equal(np.concatenate(parts), whole)
    sy.close()


def test_host_entry_equals_the_device_entry():
    M, Li, taps = 8, 4, pulse_taps(16, 0.35, 4, 0.0, 1.0)
    a, b = PfbSynthesizer(M, Li, taps, max_streams=2, max_samples=3000), PfbSynthesizer(M, Li, taps, max_streams=2, max_samples=3000)
    for sy in (a, b):
        sy.set_channels([6, 1, 2])
    for n in (3000, 3, 0, 1, 50):
        xs = np.stack([data(70 + n, 3, n), data(71 + n, 3, n)])
        got = a.work(xs)
        assert got.dtype == np.complex64 and got.shape == (2, n * Li)
        if n:
            dev = run_on_device(b, [xs[0], xs[1]])
            for s in range(2):
                assert np.array_equal(dev[s], SY.bits(got[s]).reshape(-1, 2)), (n, s)
        else:
            b.work_device(0, 0, 0, 2, 0, 0, stream())
        assert a.position() == b.position()
    one = PfbSynthesizer(M, Li, taps, max_samples=100)  # a vector per row, one stream
    want, _ = SY.synth32(taps, M, Li, data(3, M, 100))
    assert np.array_equal(SY.bits(one.work(np.array(data(3, M, 100)))[0]), SY.bits(want))
    for sy in (a, b, one):
        sy.close()


# ------------------------------------------------------------------ 5. accuracy
@pytest.mark.parametrize("M,Li,ntaps", [(8, 4, 65), (16, 16, 129), (64, 32, 513), (256, 128, 1025)])
def test_accuracy_against_the_float64_model(M, Li, ntaps):
    """|device - exact| <= gamma_q S + (1 + gamma_q) sum_k |h[n - k L]| B sqrt(M) ||a[k]||_2 per output (tests/pfbsyn_model.py (c);
    notes/pfbsyn.md has the derivation, which gives the issue's constant, and the worst ratios measured)."""
    rng = np.random.default_rng(99 + M)
    taps = (rng.normal(size=ntaps) / math.sqrt(ntaps)).astype(np.float32)
    n = 60 + 2 * -(-ntaps // Li)
    x = (rng.normal(size=(M, n)) + 1j * rng.normal(size=(M, n))).astype(np.complex64)
    sy = PfbSynthesizer(M, Li, taps, max_samples=n)
    got = run_on_device(sy, [x])[0].view(np.float32).astype(np.float64)
    got = got[:, 0] + 1j * got[:, 1]
    exact, S, A = SY.synth64(taps, M, Li, x)
    b = SY.bound(M, Li, ntaps, S, A)
    err = np.abs(got - exact)
    ratio = float((err / b).max())
    print(f"accuracy M {M} L {Li} ntaps {ntaps}: worst error / bound {ratio:.4f}, worst error {err.max():.3e}, output rms {np.sqrt(np.mean(np.abs(exact) ** 2)):.3f}")
    assert (b > 0).all() and ratio <= 1.0
    sy.close()


def test_against_the_device_route_it_replaces():
    """PfbSynthesizer(8, 4, taps) on all 8 rows against PulseShaper(4) per row, Rotator(2 pi c / 8) in place and the sum in row order:
    within the synthesizer's bound, plus per row the shaper's (gamma_terms on sum |h| |x| per component) and the rotator's
    (plcoarse_model.Rotator on the shaper's device samples), plus gamma_8 on the sum of the rows' magnitudes for the eight additions."""
    import torch
    M, Li, n = 8, 4, 1500
    taps = pulse_taps(Li, 0.2, 8)  # 65 taps
    rng = np.random.default_rng(3)
    x = (rng.normal(size=(M, n)) + 1j * rng.normal(size=(M, n))).astype(np.complex64)
    st = stream()
    sy = PfbSynthesizer(M, Li, taps, max_samples=n)
    mine = run_on_device(sy, [x])[0].view(np.float32).astype(np.float64)
    mine = mine[:, 0] + 1j * mine[:, 1]
    exact, S, A = SY.synth64(taps, M, Li, x)
    tol = SY.bound(M, Li, taps.size, S, A)
    d_sum = torch.zeros((n * Li, 2), dtype=torch.float32, device="cuda")
    magnitudes = np.zeros(n * Li)
    for c in range(M):
        ps = PulseShaper(Li, taps=taps, max_symbols=n)
        d_x = torch.from_numpy(x[c].view(np.float32).reshape(-1, 2).copy()).cuda()
        d_y = torch.zeros((n * Li, 2), dtype=torch.float32, device="cuda")
        ps.work_device(d_x.data_ptr(), n, n, 1, d_y.data_ptr(), n * Li, st)
        torch.cuda.synchronize()
        shaped = d_y.cpu().numpy().reshape(-1).view(np.complex64)
        _, mag, terms = PU.shape64(taps, Li, x[c])
        g = terms * SY.U / (1.0 - terms * SY.U)
        tol += np.hypot(g * mag[:, 0], g * mag[:, 1])
        rotated, rot_bound = PC.Rotator(2.0 * np.pi * c / M).work(shaped)
        tol += rot_bound
        magnitudes += np.abs(rotated) + rot_bound
        rot = Rotator(2.0 * np.pi * c / M)
        rot.work_device(d_y.data_ptr(), n * Li, d_y.data_ptr(), st)
        d_sum += d_y
        torch.cuda.synchronize()
        rot.close()
        ps.close()
    tol += 8 * SY.U / (1.0 - 8 * SY.U) * magnitudes
    theirs = d_sum.cpu().numpy().astype(np.float64)
    theirs = theirs[:, 0] + 1j * theirs[:, 1]
    diff = np.abs(mine - theirs)
    ratio = float((diff / tol).max())
    print(f"against the device route: worst difference / bound {ratio:.4f}, worst difference {diff.max():.3e}, output rms {np.sqrt(np.mean(np.abs(exact) ** 2)):.3f}")
    assert ratio <= 1.0 and np.abs(theirs).max() > 1000 * diff.max()
    sy.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_everything_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    good = np.ones(21, np.float32)
    gp = good.ctypes.data
    # creation (every argument refusal without a device: tests/test_pfbsyn_host.py)
    refused(capi.EINVAL, "n_chan must be a power of two in 2..256", lib.dvbs2_pfbsyn_create, C.byref(h), 6, 2, gp, 21, 1, 16, 0)
    refused(capi.EINVAL, "interp must be in 1..n_chan", lib.dvbs2_pfbsyn_create, C.byref(h), 8, 9, gp, 21, 1, 16, 0)
    refused(capi.EINVAL, "ntaps must be in 1..4096", lib.dvbs2_pfbsyn_create, C.byref(h), 8, 4, gp, 4097, 1, 16, 0)
    refused(capi.EINVAL, "n_chan * ceil(ntaps / interp) must not exceed 8192", lib.dvbs2_pfbsyn_create, C.byref(h), 256, 1, np.ones(33, np.float32).ctypes.data, 33, 1, 16, 0)
    refused(capi.EINVAL, "max_samples * interp must not exceed 2^28", lib.dvbs2_pfbsyn_create, C.byref(h), 32, 32, gp, 21, 1, (1 << 23) + 1, 0)
    refused(capi.EINVAL, "null handle pointer", lib.dvbs2_pfbsyn_create, None, 8, 4, gp, 21, 1, 16, 0)
    assert not h
    assert lib.dvbs2_pfbsyn_create(C.byref(h), 8, 4, gp, 21, 1, 16, 99) < 0 and not h  # no such device

    M, Li, n = 8, 4, 100
    taps = pulse_taps(8, 0.2, 2, 0.0, 1.0)
    sy = PfbSynthesizer(M, Li, taps, max_streams=2, max_samples=n)
    e = Expect(sy, taps, n_streams=2)
    e.set_channels([6, 1, 3])
    first, second = [data(80 + s, 3, n) for s in range(2)], [data(90 + s, 3, n) for s in range(2)]
    call(e, [x[:, :n - 1] for x in first], "before the refusals")  # (99 instants: the next outputs start off the multiples of M)
    n_out = n * Li
    d_in = torch.from_numpy(np.concatenate(second).view(np.float32)).cuda()
    d_out = sentinel(2 * (2 * n_out + PAD))
    st = stream()
    a, o = d_in.data_ptr(), d_out.data_ptr()
    count = C.c_int64(-7)
    c = C.byref(count)
    entry = lib.dvbs2_pfbsyn_process_device
    refused(capi.ESIZE, "n_in exceeds max_samples", entry, sy._h, a, n, n + 1, 2, o, n_out + Li, c, st)
    refused(capi.ESIZE, "n_streams exceeds max_streams", entry, sy._h, a, n, n, 3, o, n_out, c, st)
    refused(capi.EINVAL, "n_in is negative", entry, sy._h, a, n, -1, 2, o, n_out, c, st)
    refused(capi.EINVAL, "n_streams is negative", entry, sy._h, a, n, n, -1, o, n_out, c, st)
    refused(capi.EINVAL, "in is null", entry, sy._h, None, n, n, 2, o, n_out, c, st)
    refused(capi.EINVAL, "out is null", entry, sy._h, a, n, n, 2, None, n_out, c, st)
    refused(capi.EINVAL, "in and out must not be the same buffer", entry, sy._h, a, n, n, 2, a, n_out, c, st)
    refused(capi.EINVAL, "in_stride is below n_in", entry, sy._h, a, n - 1, n, 2, o, n_out, c, st)
    refused(capi.EINVAL, "in_stride is below n_in", entry, sy._h, a, n - 1, n, 1, o, n_out, c, st)  # one stream of three rows
    refused(capi.EINVAL, "out_stride is below n_out", entry, sy._h, a, n, n, 2, o, n_out - 1, c, st)  # before any launch
    refused(capi.EINVAL, "out_stride is below n_out", entry, sy._h, a, n, n, 1, o, n_out - 1, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, sy._h, a + 4, n, n, 2, o, n_out, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, sy._h, a, n, n, 2, o + 4, n_out, c, st)
    assert count.value == -7
    bad = np.array([5, 2, 5, 8, -1], np.int32)
    refused(capi.EINVAL, "n_sel must be in 1..n_chan", lib.dvbs2_pfbsyn_set_channels, sy._h, bad.ctypes.data, 0)
    refused(capi.EINVAL, "n_sel must be in 1..n_chan", lib.dvbs2_pfbsyn_set_channels, sy._h, bad.ctypes.data, 9)
    refused(capi.EINVAL, "null list", lib.dvbs2_pfbsyn_set_channels, sy._h, None, 2)
    refused(capi.EINVAL, "list[2] repeats a channel", lib.dvbs2_pfbsyn_set_channels, sy._h, bad.ctypes.data, 3)
    refused(capi.EINVAL, "list[1] is not a channel", lib.dvbs2_pfbsyn_set_channels, sy._h, bad[2:].ctypes.data, 2)
    refused(capi.EINVAL, "list[0] is not a channel", lib.dvbs2_pfbsyn_set_channels, sy._h, bad[4:].ctypes.data, 1)
    refused(capi.EINVAL, "counter is null", lib.dvbs2_pfbsyn_position, sy._h, None)
    assert entry(sy._h, None, 0, 0, 2, None, 0, c, st) == capi.OK  # n_in == 0: a successful call that does nothing and reports 0
    assert count.value == 0
    e.state_is("behind the refusals")
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = np.concatenate(second), np.zeros((2, n_out), np.complex64)
    count = C.c_int64(-7)
    c = C.byref(count)
    host = lib.dvbs2_pfbsyn_process
    hi, ho = host_in.ctypes.data, host_out.ctypes.data
    refused(capi.ESIZE, "n_in exceeds max_samples", host, sy._h, hi, n, n + 1, 2, ho, n_out + Li, c)
    refused(capi.EINVAL, "n_in is negative", host, sy._h, hi, n, -1, 2, ho, n_out, c)
    refused(capi.EINVAL, "in is null", host, sy._h, None, n, n, 2, ho, n_out, c)
    refused(capi.EINVAL, "out is null", host, sy._h, hi, n, n, 2, None, n_out, c)
    refused(capi.EINVAL, "in_stride is below n_in", host, sy._h, hi, n - 1, n, 2, ho, n_out, c)
    refused(capi.EINVAL, "out_stride is below n_out", host, sy._h, hi, n, n, 2, ho, n_out - 1, c)
    assert (host_out == 0).all() and count.value == -7
    # no refusal touched a tail, the counter or the selection: both streams go on from where the good call left them
    e.state_is("behind the host entry's refusals")
    call(e, second, "behind the refusals")
    # a call without streams only advances the counter
    assert sy.work_device(d_in.data_ptr(), n, 10, 0, 0, 0, st) == 10 * Li
    e.position += 10
    e.state_is("behind a call without streams")
    sy.close()


# ------------------------------------------------------------------ 7. closed loop: two carriers through synthesizer and channelizer
@functools.lru_cache(maxsize=None)
def capture():
    """The two carriers of tests/test_pfbch_gpu.py (loopback.transmit_symbols with the constants of test_ddc_gpu), here as two rows of
    PLFRAME symbols into PfbSynthesizer(8, 8, tx), tx the scaled RRC at 8 samples per symbol, set_channels([6, 1]): row 0 goes to channel
    6, row 1 to channel 1. Noise at Es/N0 = 10 dB for the power of one carrier; all of it scaled by 1 / 37.
    Returns (the encoders' inputs [2], the samples on the device, their number, symbols per carrier)."""
    import torch
    st = stream()
    sps = DG.SPS
    assert (DG.SPS, DG.ROLLOFF, DG.RRC_DELAY, DG.ES_N0_DB, DG.SCALE) == (8, 0.2, 5, 10.0, 1.0 / 37.0)
    rx = pulse_taps(sps, DG.ROLLOFF, DG.RRC_DELAY, 0.0, 1.0)
    tx = pulse_taps(sps, DG.ROLLOFF, DG.RRC_DELAY).astype(np.float64)
    tx = (tx / np.convolve(tx, rx.astype(np.float64))[2 * sps * DG.RRC_DELAY]).astype(np.float32)
    sent, rows, n_all = [], [], None
    for k in range(2):
        sent_k, d_x, n, n_all_k, _ = L.transmit_symbols(DG.SEQ, DG.ND, L.GOLD, DG.LEAD, seed=3000 + k, flush=256)
        assert n_all in (None, n_all_k)
        n_all = n_all_k
        sent.append(sent_k)
        rows.append(d_x)
    d_rows = torch.stack(rows).contiguous()  # [2, n_all, 2]
    ns = n_all * sps
    sy = PfbSynthesizer(8, 8, tx, max_samples=n_all)
    sy.set_channels([6, 1])
    d_wide = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
    assert sy.work_device(d_rows.data_ptr(), n_all, n_all, 1, d_wide.data_ptr(), ns, st) == ns
    torch.cuda.synchronize()
    sy.close()
    # one carrier's power: a row on its own through the same taps (the shaper's sum, whatever the channel)
    ps = PulseShaper(sps, taps=tx, max_symbols=n_all)
    d_y = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
    ps.work_device(rows[0].data_ptr(), n_all, n_all, 1, d_y.data_ptr(), ns, st)
    power = float((d_y[:n * sps] ** 2).sum(dim=1).mean().item())
    both = float((d_wide[:n * sps] ** 2).sum(dim=1).mean().item())
    ps.close()
    assert abs(both / (2 * power) - 1) < 0.05
    noise = Awgn(seed=77, sigma=awgn_sigma(DG.ES_N0_DB, es=power, sps=sps), max_samples=ns)
    noise.work_device(d_wide.data_ptr(), ns, ns, 1, d_wide.data_ptr(), ns, first_index=0, stream=st)
    d_wide *= DG.SCALE
    torch.cuda.synchronize()
    noise.close()
    return sent, d_wide, ns, n_all


def channelize(sel):
    import torch
    sent, d_wide, ns, n_all = capture()
    ch = PfbChannelizer(8, 4, pulse_taps(8, 0.2, 5, 0, 1), max_samples=ns)
    ch.set_channels(sel)
    n_out = ch.produce(ns)
    assert n_out == ns // 4  # 2 samples per symbol
    d_rows = torch.zeros((len(sel), n_out, 2), dtype=torch.float32, device="cuda")
    assert ch.work_device(d_wide.data_ptr(), ns, ns, 1, d_rows.data_ptr(), n_out, stream()) == n_out
    torch.cuda.synchronize()
    ch.close()
    return sent, d_rows, n_out, n_all


def receive_every_frame(d_y, ns, n_syms, what):
    """test_ddc_gpu.receive once more, for ALL data frames. That receive side decodes the frames the tracker reports as locked, and the
    tracker locks at the SECOND header it meets: the first data frame behind the lead is found (its record is there, with its PLSC and
    its SOF) but is not among the gathered ones. Here the same stages run again and the first frame's record is marked for the
    gather as well, so that loopback.decode_frames takes every data frame. Returns (messages, which data frame each is)."""
    import torch
    st = stream()
    reference = float(torch.linalg.vector_norm(d_y[:2 * DG.LEAD], dim=1).mean().item()) / DG.SCALE
    agc = Agc(rate=0.05, reference=reference, gain=1.0, max_gain=65536.0, max_samples=ns)
    d_g = torch.zeros_like(d_y)
    d_gain = torch.zeros(ns, dtype=torch.float32, device="cuda")
    agc.work_device(d_y.data_ptr(), ns, ns, 1, d_g.data_ptr(), ns, d_gain.data_ptr(), ns, st)
    rx = L.timing_and_frames(d_g, ns, 2, DG.ROLLOFF, SymbolSync.CUBIC, n_syms, tol=24)
    recs = rx.recs.copy()
    behind = np.nonzero(recs["sof_index"] >= DG.LEAD)[0]
    assert rx.state == capi.PLSYNC_LOCKED and recs["plsc"][behind].tolist() == DG.SEQ, what
    first = int(behind[0])
    assert all(recs["flags"][f] & capi.PLSYNC_FLAG_LOCKED for f in behind[1:]), what
    recs["flags"][first] |= capi.PLSYNC_FLAG_LOCKED
    raw = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    rx.d_rec[:raw.numel()] = raw
    got = L.decode_frames(rx._replace(recs=recs), DG.PLSC, L.GOLD, 10 ** (-DG.ES_N0_DB / 10), first_sof=DG.LEAD)
    rx.sync.close()
    agc.close()
    return got.msg, got.data_index


def test_closed_loop_each_row_returns_what_its_synthesizer_row_was_fed():
    """Channelizer set_channels([6, 1]): row 0 returns the bytes fed to synthesizer row 0, row 1 those of row 1, neither the other's: the
    sign of the transform and the order of the selection are the channelizer's. First through the receive side of test_ddc_gpu as it
    is (the frames its tracker locked on), then through the same stages for ALL data frames of both carriers: none is left out."""
    sent, d_rows, n_out, n_all = channelize([6, 1])
    for row in range(2):
        msg, data_index = DG.receive(d_rows[row], n_out, n_all, f"row {row}")
        assert np.array_equal(msg, sent[row][data_index]), row  # the encoder's input bytes
        assert not np.array_equal(msg, sent[row ^ 1][data_index])
        msg, data_index = receive_every_frame(d_rows[row], n_out, n_all, f"row {row}, every frame")
        assert [int(i) for i in data_index] == list(range(DG.ND)), (row, data_index)
        assert np.array_equal(msg, sent[row]) and not np.array_equal(msg, sent[row ^ 1]), row


def test_closed_loop_the_mirror_channels_hold_no_carrier():
    """Channelizer set_channels([7, 2]), the mirror images of channels 1 and 6: behind the same AGC and timing recovery the frame search
    does not reach PLSYNC_LOCKED on either row."""
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
        assert state != capi.PLSYNC_LOCKED and nf == 0
