"""Digital down-converter on the device (dvbs2_ddc_*). The expected output of a channel is model (a) of tests/ddc_model.py applied to
what Rotator gives ON THE DEVICE for the same input and increment: every output sample BIT FOR BIT (uint32 compare) into sentinel-filled
buffers whose pads and gaps must stay untouched, with zeros of both signs and denormals planted in the input; the device's phases and the
host's mirror against Python integers after every call; the device against the float64 model under a derived bound; and a closed loop:
two carriers in one band, each back through its own channel and the receive stages of this library."""
import ctypes as C
import functools

import numpy as np
import pytest

import ddc_model as DM
import fec_testlib as T
import loopback as L
import plcoarse_model as PC
import pulse_model as PM
from dvbs2rx_amd import Agc, Awgn, Ddc, PulseShaper, Rotator, SymbolSync, awgn_sigma, capi, ddc_tile, plframer_layout, pulse_taps
from fec_testlib import PAD, SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def data(seed, n):
    x = PM.planted(np.random.default_rng(seed), n)
    x.setflags(write=False)
    return x


def rotate_on_device(rot, x):
    """what the rotator stage gives on the device for the host samples x, continuing from the handle's phase"""
    import torch
    if x.size == 0:
        return np.zeros(0, np.complex64)
    d_x = torch.from_numpy(np.array(x, np.complex64).view(np.float32)).cuda()  # (a copy: the cached data are read-only)
    d_z = torch.empty_like(d_x)
    rot.work_device(d_x.data_ptr(), x.size, d_z.data_ptr(), stream())
    torch.cuda.synchronize()
    return d_z.cpu().numpy().view(np.complex64)


def inc_turns_exact(inc):
    """the increment in 2^-64 turns from exact arithmetic, rounded to nearest"""
    return ((PC.turns(inc) + (1 << (PC.FRAC - 65))) >> (PC.FRAC - 64)) & MASK


class Expect:
    """what a handle with these channels must write and hold: per channel a Rotator on the device, model (a) with its history, and the
    64-bit phase in Python integers; the sample counter they share"""

    def __init__(self, dd, taps, chans):
        self.dd, self.taps, self.D = dd, np.ascontiguousarray(taps, np.float32), dd.decim
        self.inputs = [i for i, _ in chans]
        self.rots = [Rotator(inc) for _, inc in chans]
        self.incs = [0] * len(chans)
        self.hist, self.phase, self.position = [None] * len(chans), [0] * len(chans), 0
        for c, (i, inc) in enumerate(chans):
            self.set_channel(c, inc, i, rotator_too=False)

    def set_channel(self, c, inc, input=None, rotator_too=True):
        self.inputs[c] = self.inputs[c] if input is None else input
        self.dd.set_channel(c, inc, self.inputs[c])
        got_input, got_inc, _ = self.dd.channel(c)
        d = (got_inc - inc_turns_exact(inc)) & MASK
        assert got_input == self.inputs[c] and min(d, (1 << 64) - d) <= 2, (got_inc, inc_turns_exact(inc))  # the conversion's own error
        self.incs[c] = got_inc
        if rotator_too:
            self.rots[c].set_phase_inc(inc)

    def reset(self):
        self.dd.reset()
        for r in self.rots:
            r.reset()  # (back to the constructor's increment: callers that changed one set it again)
        self.hist, self.phase, self.position = [None] * len(self.rots), [0] * len(self.rots), 0

    def work(self, xs, n_channels):
        n, outs = xs[0].size, []
        for c in range(n_channels):
            z = rotate_on_device(self.rots[c], xs[self.inputs[c]])
            y, self.hist[c] = DM.decimate32(self.taps, self.D, z, self.position, self.hist[c])
            self.phase[c] = DM.phase_after(self.phase[c], self.incs[c], n)
            outs.append(y)
        self.position += n
        return outs

    def state_is(self, what):
        """the device's phases, the host's mirror and the counter against the Python integers"""
        dd = self.dd
        assert [int(p) for p in dd.state()[:len(self.phase)]] == self.phase, what
        assert [dd.channel(c)[2] for c in range(len(self.phase))] == self.phase and dd.position() == self.position, what
        for n_in in (0, 1, min(97, dd.max_samples)):
            assert dd.produce(n_in) == DM.produce(self.position, self.D, n_in), what

    def close(self):
        for r in self.rots:
            r.close()
        self.dd.close()


def run_on_device(dd, xs, n_channels, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the input streams xs (complex64 vectors of one length n) through fec_testlib.run_strided: input i lies at
    in_shift + i * in_stride complex elements of the input buffer, channel c writes at out_shift + c * out_stride of a sentinel buffer.
    Returns one uint32 (n_out, 2) array per channel after checking that the reported count is what produce() gave before the call."""
    ni, n = len(xs), xs[0].size
    said = dd.produce(n)
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(said, 1) if out_stride is None else out_stride
    outs, n_out = T.run_strided(lambda a, o: dd.work_device(a, in_stride, n, ni, n_channels, o, out_stride, stream()), xs, [said] * n_channels,
                                in_stride, out_stride, in_shift, out_shift)
    assert n_out == said == DM.produce(dd.position() - n, dd.decim, n)
    return outs


def same(got, want, what):
    T.same_bits(got, DM.bits(want), what)


def call(e, xs, n_channels, what, **where):
    got = run_on_device(e.dd, xs, n_channels, **where)
    want = e.work(xs, n_channels)
    for c in range(n_channels):
        same(got[c], want[c], f"{what}, channel {c}")
    e.state_is(what)
    return got


# ------------------------------------------------------------------ 1. bit for bit over decimations, filter lengths and tile edges
def _shapes():
    out = []
    for D in (1, 2, 3, 8, 256):
        for ntaps in sorted({1, D - 1, D, D + 1, 2 * D + 1, 4096}):
            if ntaps >= 1:
                out.append((D, ntaps))
    return out


@pytest.mark.parametrize("D,ntaps", _shapes())
def test_bit_for_bit_at_the_tile_edges(D, ntaps):
    """Two channels on one input, increments 0 (no special case: the signs of zeros are the rotator's) and -1.234567. From a reset
    handle the shortest calls that write tile - 1, tile, tile + 1 and 2 tile + 3 outputs, each followed by calls of 0, 1, D - 1 and 40
    samples that go on from its history (shorter than the history: old history and input both enter the new one) and from positions that
    are no multiples of D."""
    rng = np.random.default_rng(1000 * D + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    tile = ddc_tile(D, ntaps)
    targets = (tile - 1, tile, tile + 1, 2 * tile + 3)
    dd = Ddc(D, taps, max_channels=2, max_samples=(targets[-1] - 1) * D + 1)
    assert (dd.decim, dd.ntaps, dd.history, dd.delay_num, dd.tile) == (D, ntaps, ntaps - 1, ntaps - 1, tile)
    e = Expect(dd, taps, [(0, 0.0), (0, -1.234567)])
    for target in targets:
        e.reset()
        n_in = (target - 1) * D + 1  # the first output uses the first sample, the last output the last
        assert DM.produce(0, D, n_in) == target and DM.produce(0, D, n_in - 1) == target - 1
        call(e, [data(D * 10000 + n_in % 9973, n_in)], 2, f"D {D} ntaps {ntaps}: {target} outputs")
        for more in (0, 1, D - 1, 40):
            call(e, [data(7 + more, max(more, 1))[:more]], 2, f"D {D} ntaps {ntaps}: {more} samples behind {target} outputs")
    e.reset()
    for first in (0, 1, D - 1):  # the same short calls on a handle that has nothing but zeros behind it
        call(e, [data(17 + first, max(first, 1))[:first]], 2, f"D {D} ntaps {ntaps}: {first} samples from a reset handle")
    e.close()


@pytest.mark.parametrize("D,ntaps", [(8, 129), (50, 801), (10, 1001), (20, 201), (4, 65)])
def test_designed_filters(D, ntaps):
    """The shapes of the timing tool and the three builds of the kernel: tiles of 1024 (four outputs per lane), 168 (one), 821 (four,
    the last of them past the tile's end for most lanes), 450 (two) and 1024."""
    assert ddc_tile(D, ntaps) == {(8, 129): 1024, (50, 801): 168, (10, 1001): 821, (20, 201): 450, (4, 65): 1024}[(D, ntaps)]
    rng = np.random.default_rng(D)
    taps = (np.sinc((np.arange(ntaps) - (ntaps - 1) / 2) / D) * np.hamming(ntaps) / D).astype(np.float32)
    tile = ddc_tile(D, ntaps)
    n_in = (2 * tile + 77) * D - 3
    dd = Ddc(D, taps, max_channels=3, max_samples=n_in)
    e = Expect(dd, taps, [(0, float(rng.uniform(-3, 3))) for _ in range(3)])
    call(e, [data(31 + D, n_in)], 3, f"D {D} ntaps {ntaps}: first call")
    call(e, [data(32 + D, 3 * D + 1)], 3, f"D {D} ntaps {ntaps}: second call")
    e.close()


@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_alignment_and_strides(in_shift, out_shift):
    """Buffers displaced by one complex element are 8-byte but not 16-byte aligned, and strides larger than needed: the same bits."""
    D, ntaps = 3, 7
    taps = np.random.default_rng(5).normal(size=ntaps).astype(np.float32)
    n_in = 3 * ddc_tile(D, ntaps) // 2 * D + 1
    dd = Ddc(D, taps, max_channels=3, max_inputs=2, max_samples=n_in)
    e = Expect(dd, taps, [(1, 0.3), (0, -0.3), (1, 2.9)])
    xs = [data(60, n_in), data(61, n_in)]
    call(e, xs, 3, f"shifts {in_shift} {out_shift}", in_stride=n_in + 3 + (in_shift ^ 1), out_stride=dd.produce(n_in) + 5 + out_shift,
         in_shift=in_shift, out_shift=out_shift)
    e.close()


# ------------------------------------------------------------------ 2. cuts
@pytest.mark.parametrize("D,ntaps", [(8, 129), (3, 2), (256, 300)])
def test_cuts_give_the_bits_of_one_call(D, ntaps):
    """A stream in one call equals the same stream in random cuts, one of them without an output, with an increment change between two
    cuts; state() and position() equal the mirror after every call (call() checks them)."""
    rng = np.random.default_rng(D + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    tile = ddc_tile(D, ntaps)
    n = (2 * tile + 5) * D + D // 2
    x = data(40 + D, n)
    dd = Ddc(D, taps, max_channels=2, max_samples=n)
    e = Expect(dd, taps, [(0, 0.7), (0, -2.2)])
    whole = call(e, [x], 2, "one call")
    e.reset()
    # 1, 0, D - 1, D + 1 samples bring the counter to 2 D + 1; one more sample from there lies between two outputs (at D = 1 every
    # sample is an output, and only the empty cut writes none)
    cuts = [1, 0, D - 1, D + 1, 1] + [int(c) for c in rng.integers(1, tile * D // 2, 3)]
    assert sum(cuts) < n
    cuts.append(n - sum(cuts))
    parts, pos, saw_empty = [[], []], 0, False
    for c in cuts:
        saw_empty |= DM.produce(e.position, D, c) == 0 and (c > 0 or D == 1)
        got = call(e, [x[pos:pos + c]], 2, f"cut of {c} at {pos}")
        for ch in range(2):
            parts[ch].append(got[ch])
        pos += c
    assert pos == n and saw_empty
    for ch in range(2):
        assert np.array_equal(np.concatenate(parts[ch]), whole[ch]), cuts
    # an increment change between two cuts: the phase stays continuous, the history keeps what was mixed with the old increment
    e.set_channel(0, -0.45)
    call(e, [data(41, 5 * D + 3)], 2, "behind set_channel")
    e.set_channel(1, 0.0)
    call(e, [data(42, 2 * D)], 2, "behind the second set_channel")
    e.close()


# ------------------------------------------------------------------ 3. channels and inputs
def test_channels_and_inputs():
    """5 channels on 2 inputs; channels 1 and 3 share an input and an increment and must agree; each channel equals a one-channel
    handle; a call on 3 of the 5 channels leaves the state of the other two alone."""
    D, ntaps = 4, 33
    taps = pulse_taps(8, 0.2, 2, 0.0, 1.0)
    assert taps.size == ntaps
    chans = [(0, 0.5), (1, -0.9), (0, 0.0), (1, -0.9), (1, 3.0)]
    n = 2 * ddc_tile(D, ntaps) * D // 3 + 2
    xs = [data(50, n), data(51, n)]
    dd = Ddc(D, taps, max_channels=5, max_inputs=2, max_samples=n)
    e = Expect(dd, taps, chans)
    first = call(e, xs, 5, "five channels", in_stride=n + 1)
    assert np.array_equal(first[1], first[3]) and not np.array_equal(first[1], first[4]) and not np.array_equal(first[0], first[2])
    for c, (i, inc) in enumerate(chans):
        one = Ddc(D, taps, max_samples=n)
        one.set_channel(0, inc)
        got = run_on_device(one, [xs[i]], 1)[0]
        assert np.array_equal(got, first[c]), c
        one.close()
    before = dd.state().copy()
    call(e, [x[:77] for x in xs], 3, "three of five channels", in_stride=80)
    after = dd.state()
    assert np.array_equal(after[3:], before[3:]) and not np.array_equal(after[:3], before[:3])
    # the two channels left out go on from their own histories and phases, 77 samples late
    call(e, [x[77:200] for x in xs], 5, "all five again", in_stride=123)
    e.close()


def test_host_entry_equals_the_device_entry():
    D, taps = 8, pulse_taps(16, 0.35, 4, 0.0, 1.0)
    a, b = Ddc(D, taps, max_channels=2, max_inputs=2, max_samples=3000), Ddc(D, taps, max_channels=2, max_inputs=2, max_samples=3000)
    for dd in (a, b):
        dd.set_channel(0, 0.8, 1)
        dd.set_channel(1, -0.1, 0)
    for n in (3000, 3, 0, 1, 50):
        xs = np.stack([data(70 + n, max(n, 1))[:n], data(71 + n, max(n, 1))[:n]])
        got = a.work(xs)
        assert got.dtype == np.complex64 and got.shape == (2, DM.produce(b.position(), D, n))
        if n:
            dev = run_on_device(b, [xs[0], xs[1]], 2)
            for c in range(2):
                assert np.array_equal(dev[c], DM.bits(got[c]).reshape(-1, 2)), (n, c)
        assert np.array_equal(a.state(), b.state()) and a.position() == b.position()
    a.close()
    b.close()


# ------------------------------------------------------------------ 4. accuracy
def test_accuracy_against_the_float64_model():
    """|device - exact| per component is at most
        sum_t |h[t]| B[k D - t]  +  gamma_ntaps sum_t |h[t]| |z[k D - t]|,
    B the rotator's per-sample bound on |z_device - z_exact| (plcoarse_model.Rotator.work: phase representation, the increment's
    rounding, sincospif, the complex product; it bounds the modulus, hence each component), gamma_n = n u / (1 - n u) the bound of a
    recursive sum of n rounded products (tests/test_ddc_model.py), z the mixed float32 samples. notes/ddc.md has the derivation and the
    worst ratio measured."""
    D, inc = 8, 0.6180339887
    taps = pulse_taps(16, 0.35, 4, 0.0, 1.0)
    ntaps = taps.size
    rng = np.random.default_rng(99)
    x = (rng.normal(size=6000) + 1j * rng.normal(size=6000)).astype(np.complex64)
    dd = Ddc(D, taps, max_samples=x.size)
    dd.set_channel(0, inc)
    got = run_on_device(dd, [x], 1)[0].view(np.float32)
    exact, mix_bound = DM.ddc64(taps, D, x, inc)
    rot = Rotator(inc)
    z = rotate_on_device(rot, x)
    rot.close()
    _, mag = DM.decimate64(taps, D, z)
    gamma = ntaps * DM.U / (1.0 - ntaps * DM.U)
    err = np.stack([np.abs(got[:, 0].astype(np.float64) - exact.real), np.abs(got[:, 1].astype(np.float64) - exact.imag)], axis=1)
    bound = mix_bound[:, None] + gamma * mag
    ratio = (err / bound).max()
    print(f"accuracy: worst error / bound {ratio:.4f}, worst error {err.max():.3e}, output rms {np.sqrt(np.mean(np.abs(exact) ** 2)):.3f}")
    assert ratio <= 1.0
    dd.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_everything_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    good = np.ones(21, np.float32)
    # creation (every argument refusal without a device: tests/test_ddc_model.py)
    refused(capi.EINVAL, "decim must be in 1..256", lib.dvbs2_ddc_create, C.byref(h), 0, good.ctypes.data, 21, 1, 1, 16, 0)
    refused(capi.EINVAL, "ntaps must be in 1..4096", lib.dvbs2_ddc_create, C.byref(h), 4, good.ctypes.data, 4097, 1, 1, 16, 0)
    refused(capi.EINVAL, "null handle pointer", lib.dvbs2_ddc_create, None, 4, good.ctypes.data, 21, 1, 1, 16, 0)
    assert not h
    assert lib.dvbs2_ddc_create(C.byref(h), 4, good.ctypes.data, 21, 1, 1, 16, 99) < 0 and not h  # no such device

    D, n = 4, 100
    taps = pulse_taps(8, 0.2, 2, 0.0, 1.0)
    dd = Ddc(D, taps, max_channels=2, max_inputs=2, max_samples=n)
    e = Expect(dd, taps, [(0, 0.4), (1, -0.4)])
    first, second = [data(80 + s, n) for s in range(2)], [data(90 + s, n) for s in range(2)]
    call(e, [x[:n - 1] for x in first], 2, "before the refusals")  # (99 samples: the counter is no multiple of D)
    n_out = dd.produce(n)
    assert n_out == DM.produce(n - 1, D, n) == 25
    d_in = torch.from_numpy(np.concatenate(second).view(np.float32)).cuda()
    d_out = sentinel(2 * (2 * n_out + PAD))
    st = stream()
    a, o = d_in.data_ptr(), d_out.data_ptr()
    count = C.c_int64(-7)
    c = C.byref(count)
    entry = lib.dvbs2_ddc_process_device
    refused(capi.ESIZE, "n_in exceeds max_samples", entry, dd._h, a, n, n + 1, 2, 2, o, n_out, c, st)
    refused(capi.ESIZE, "n_inputs exceeds max_inputs", entry, dd._h, a, n, n, 3, 2, o, n_out, c, st)
    refused(capi.ESIZE, "n_channels exceeds max_channels", entry, dd._h, a, n, n, 2, 3, o, n_out, c, st)
    refused(capi.EINVAL, "n_in is negative", entry, dd._h, a, n, -1, 2, 2, o, n_out, c, st)
    refused(capi.EINVAL, "n_inputs is negative", entry, dd._h, a, n, n, -1, 2, o, n_out, c, st)
    refused(capi.EINVAL, "n_channels is negative", entry, dd._h, a, n, n, 2, -1, o, n_out, c, st)
    refused(capi.EINVAL, "in is null", entry, dd._h, None, n, n, 2, 2, o, n_out, c, st)
    refused(capi.EINVAL, "out is null", entry, dd._h, a, n, n, 2, 2, None, n_out, c, st)
    refused(capi.EINVAL, "channel 1 reads input 1, which is not below n_inputs", entry, dd._h, a, n, n, 1, 2, o, n_out, c, st)
    refused(capi.EINVAL, "in_stride is below n_in", entry, dd._h, a, n - 1, n, 2, 2, o, n_out, c, st)
    refused(capi.EINVAL, "out_stride is below n_out", entry, dd._h, a, n, n, 2, 2, o, n_out - 1, c, st)  # before any launch
    refused(capi.EINVAL, "out_stride is below n_out", entry, dd._h, a, n, n, 2, 1, o, n_out - 1, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, dd._h, a + 4, n, n, 2, 2, o, n_out, c, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, dd._h, a, n, n, 2, 2, o + 4, n_out, c, st)
    assert count.value == -7
    refused(capi.EINVAL, "channel out of range", lib.dvbs2_ddc_set_channel, dd._h, 2, 0, 0.1)
    refused(capi.EINVAL, "channel out of range", lib.dvbs2_ddc_set_channel, dd._h, -1, 0, 0.1)
    refused(capi.EINVAL, "input out of range", lib.dvbs2_ddc_set_channel, dd._h, 0, 2, 0.1)
    refused(capi.EINVAL, "input out of range", lib.dvbs2_ddc_set_channel, dd._h, 0, -1, 0.1)
    refused(capi.EINVAL, "phase_inc must be finite", lib.dvbs2_ddc_set_channel, dd._h, 0, 0, float("nan"))
    refused(capi.EINVAL, "phase_inc must be finite", lib.dvbs2_ddc_set_channel, dd._h, 0, 0, float("inf"))
    refused(capi.EINVAL, "channel out of range", lib.dvbs2_ddc_channel, dd._h, 2, None, None, None)
    refused(capi.EINVAL, "counter is null", lib.dvbs2_ddc_position, dd._h, None)
    refused(capi.EINVAL, "phases is null", lib.dvbs2_ddc_state, dd._h, None)
    assert entry(dd._h, None, 0, 0, 2, 2, None, 0, c, st) == capi.OK  # n_in == 0: a successful call that does nothing and reports 0
    assert count.value == 0
    e.state_is("behind the refusals")
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = np.stack(second), np.zeros((2, n_out), np.complex64)
    count = C.c_int64(-7)
    c = C.byref(count)
    host = lib.dvbs2_ddc_process
    hi, ho = host_in.ctypes.data, host_out.ctypes.data
    refused(capi.ESIZE, "n_in exceeds max_samples", host, dd._h, hi, n, n + 1, 2, 2, ho, n_out, c)
    refused(capi.EINVAL, "n_in is negative", host, dd._h, hi, n, -1, 2, 2, ho, n_out, c)
    refused(capi.EINVAL, "in is null", host, dd._h, None, n, n, 2, 2, ho, n_out, c)
    refused(capi.EINVAL, "out is null", host, dd._h, hi, n, n, 2, 2, None, n_out, c)
    refused(capi.EINVAL, "in_stride is below n_in", host, dd._h, hi, n - 1, n, 2, 2, ho, n_out, c)
    refused(capi.EINVAL, "out_stride is below n_out", host, dd._h, hi, n, n, 2, 2, ho, n_out - 1, c)
    assert (host_out == 0).all() and count.value == -7
    # no refusal touched a history, a phase or the mirror: both channels go on from where the good call left them
    e.state_is("behind the host entry's refusals")
    call(e, second, 2, "behind the refusals")
    # a call without channels only advances the counter
    assert dd.work_device(d_in.data_ptr(), n, 10, 2, 0, 0, 0, st) == DM.produce(e.position, D, 10)
    e.position += 10
    e.state_is("behind a call without channels")
    e.close()


# ------------------------------------------------------------------ 6. closed loop: two carriers in one band
PLSC, ND, LEAD = L.PLSC, 4, 2001
SEQ = [PLSC, PLSC, L.DUMMY, PLSC, PLSC]  # a dummy frame after data frame 2
SPS, ROLLOFF, RRC_DELAY, SPACING = 8, 0.2, 5, 1.5
ES_N0_DB = 10.0  # the chain alone decodes QPSK 1/4 short without an error from 1 dB on (tests/test_awgn_gpu.py)
SCALE = 1.0 / 37.0  # the capture is weak: the AGC behind the down-converter has to bring it back
CARRIER_INC = 2 * np.pi * (SPACING / 2) / SPS  # +-0.75 symbol rates in radians per sample


@functools.lru_cache(maxsize=None)
def capture():
    """Two carriers of short QPSK 1/4 frames with different payloads (loopback.transmit_symbols, 256 zero symbols of flush: more than the
    histories of all stages behind), each shaped at 8 samples per symbol (taps scaled so that the symbols behind the channel filter have
    unit amplitude), moved to -+0.75 symbol rates and added; noise at Es/N0 = ES_N0_DB for the power of one carrier; all of it scaled by
    SCALE. Returns (the encoders' inputs [2], the samples on the device, their number, symbols per carrier)."""
    import torch
    st = stream()
    rx = pulse_taps(SPS, ROLLOFF, RRC_DELAY, 0.0, 1.0)
    tx = pulse_taps(SPS, ROLLOFF, RRC_DELAY).astype(np.float64)
    tx = (tx / np.convolve(tx, rx.astype(np.float64))[2 * SPS * RRC_DELAY]).astype(np.float32)
    d_sum, sent, power = None, [], []
    for k, sign in enumerate((-1.0, 1.0)):
        sent_k, d_x, n, n_all, _ = L.transmit_symbols(SEQ, ND, L.GOLD, LEAD, seed=3000 + k, flush=256)
        sent.append(sent_k)
        ns = n_all * SPS
        ps = PulseShaper(SPS, taps=tx, max_symbols=n_all)
        d_y = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
        ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), ns, st)
        power.append(float((d_y[:n * SPS] ** 2).sum(dim=1).mean().item()))
        rot = Rotator(sign * CARRIER_INC)
        rot.work_device(d_y.data_ptr(), ns, d_y.data_ptr(), st)
        if d_sum is None:
            d_sum = torch.zeros_like(d_y)
        d_sum += d_y
        torch.cuda.synchronize()
        rot.close()
        ps.close()
    assert abs(power[0] / power[1] - 1) < 0.05
    noise = Awgn(seed=77, sigma=awgn_sigma(ES_N0_DB, es=power[0], sps=SPS), max_samples=ns)
    noise.work_device(d_sum.data_ptr(), ns, ns, 1, d_sum.data_ptr(), ns, first_index=0, stream=st)
    d_sum *= SCALE
    torch.cuda.synchronize()
    noise.close()
    return sent, d_sum, ns, n_all


def receive(d_y, ns, n_syms, what):
    """d_y: ns samples of one channel at 2 per symbol on the device, behind the channel filter. AGC, timing recovery with the cubic
    interpolator (the matched filter is already applied), frame search and the decode tail of tests/loopback.py. Returns the messages of
    the frames the tracker locked on and which encoder frame each carries."""
    import torch
    st = stream()
    lay = plframer_layout(SEQ)
    # the reference: the mean magnitude of the channel's samples at full scale, so that the settled gain is 1 / SCALE and the symbols
    # come out at the unit amplitude they were sent with
    reference = float(torch.linalg.vector_norm(d_y[:2 * LEAD], dim=1).mean().item()) / SCALE
    agc = Agc(rate=0.05, reference=reference, gain=1.0, max_gain=65536.0, max_samples=ns)
    d_g = torch.zeros_like(d_y)
    d_gain = torch.zeros(ns, dtype=torch.float32, device="cuda")
    agc.work_device(d_y.data_ptr(), ns, ns, 1, d_g.data_ptr(), ns, d_gain.data_ptr(), ns, st)
    rx = L.timing_and_frames(d_g, ns, 2, ROLLOFF, SymbolSync.CUBIC, n_syms, tol=24)
    recs = rx.recs
    settled = d_gain[2 * LEAD:2 * (LEAD + lay["out_syms"])].cpu().numpy()
    print(f"{what}: AGC gain behind the lead {settled.min():.2f} .. {settled.max():.2f}, {rx.nsym} symbols from {ns} samples ({n_syms} sent), "
          f"status 0")  # (a status other than 0 does not come back from timing_and_frames)
    assert 0.8 / SCALE < settled.min() and settled.max() < 1.25 / SCALE, what
    behind = recs[recs["sof_index"] >= LEAD]
    shifts = (behind["sof_index"] - (LEAD + lay["out_offset"][:behind.size])).tolist() if behind.size <= len(SEQ) else []
    print(f"{what}: {rx.nf} frames, PLSCs behind the lead {behind['plsc'].tolist()}, SOF shifts {shifts}")
    assert rx.state == capi.PLSYNC_LOCKED and behind["plsc"].tolist() == SEQ, what  # every frame behind the lead is found
    assert len(set(shifts)) == 1 and abs(shifts[0] - 2 * RRC_DELAY) <= 12, (what, shifts)  # the shaper's and the channel filter's delay
    got = L.decode_frames(rx, PLSC, L.GOLD, 10 ** (-ES_N0_DB / 10), first_sof=LEAD)
    assert len(got.locked) >= ND - 1 and len(got.locked) == sum(1 for r in recs if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == PLSC), what
    rx.sync.close()
    agc.close()
    return got.msg, got.data_index


@pytest.mark.parametrize("swapped", [False, True])
def test_closed_loop_two_carriers(swapped):
    """One handle with D = 4 and dvbs2_pulse_taps(8, 0.2, 5, 0, 1) as channel filter brings both carriers to 2 samples per symbol; each
    channel returns its own encoder's input bytes. With the two increments swapped each channel returns the OTHER carrier's bytes: the
    sign of the mixer is pinned."""
    import torch
    sent, d_wide, ns, n_all = capture()
    taps = pulse_taps(SPS, ROLLOFF, RRC_DELAY, 0.0, 1.0)
    dd = Ddc(SPS // 2, taps, max_channels=2, max_samples=ns)
    # carrier k sits at (-1, +1)[k] CARRIER_INC: channel k brings it to 0 with the opposite increment
    incs = [CARRIER_INC, -CARRIER_INC]
    if swapped:
        incs.reverse()
    for c in range(2):
        dd.set_channel(c, incs[c])
    n_out = dd.produce(ns)
    assert n_out == ns // 4
    d_ch = torch.zeros((2, n_out, 2), dtype=torch.float32, device="cuda")
    assert dd.work_device(d_wide.data_ptr(), ns, ns, 1, 2, d_ch.data_ptr(), n_out, stream()) == n_out
    torch.cuda.synchronize()
    for c in range(2):
        carrier = c ^ int(swapped)
        msg, data_index = receive(d_ch[c], n_out, n_all, f"channel {c} (carrier {carrier})")
        assert np.array_equal(msg, sent[carrier][data_index]), (c, swapped)  # the encoder's input bytes
        assert not np.array_equal(msg, sent[carrier ^ 1][data_index])
    dd.close()
