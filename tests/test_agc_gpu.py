"""AGC on the device (dvbs2_agc_*) against the float32 model of tests/agc_model.py: every output sample, every gain and the gains the
handle keeps BIT FOR BIT (uint32 compare; where the model has a NaN the device must have one), into sentinel-filled buffers whose pads
and gaps must stay untouched; then the receive stages of this library in a closed loop behind it."""
import ctypes as C
import functools

import numpy as np
import pytest

import agc_model as AM
import loopback as L
from dvbs2rx_amd import Agc, capi
from fec_testlib import SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu

PAD = 64               # sentinel elements behind the last stream
T = capi.AGC_TILE      # the kernel's tile in samples


def run(agc, x, with_gain=True, in_stride=None, out_stride=None, gain_stride=None, in_shift=0, out_shift=0, in_place=False):
    """One work_device call over the streams x (complex64 [ns, n]). Stream s lies at in_shift + s * in_stride complex elements of a
    16-byte-aligned input buffer and is written at out_shift + s * out_stride of a 16-byte-aligned sentinel buffer (in place: into the
    input buffer), its gains at s * gain_stride floats of a third. Returns (uint32 [ns, 2 n] samples, uint32 [ns, n] gains or None) after
    checking that everything else in the buffers is still what it was."""
    import torch
    ns, n = x.shape
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = (in_stride if in_place else max(n, 1)) if out_stride is None else out_stride
    gain_stride = max(n, 1) if gain_stride is None else gain_stride
    host_in = np.full(in_shift + ns * in_stride + PAD, np.complex64(complex(9.5, -9.5)), np.complex64)
    for s in range(ns):
        host_in[in_shift + s * in_stride:in_shift + s * in_stride + n] = x[s]
    d_in = torch.from_numpy(host_in.view(np.float32)).cuda()
    n_out = out_shift + (ns - 1) * out_stride + n + PAD
    d_out = d_in if in_place else sentinel(2 * n_out)
    n_gain = (ns - 1) * gain_stride + n + PAD
    d_gain = sentinel(n_gain) if with_gain else None
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    agc.work_device(d_in.data_ptr() + 8 * in_shift, in_stride, n, ns, d_out.data_ptr() + 8 * (in_shift if in_place else out_shift), out_stride,
                    d_gain.data_ptr() if with_gain else 0, gain_stride, stream())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    if in_place:
        out_shift, before = in_shift, host_in.view(np.uint32).reshape(-1, 2)
    else:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), host_in.view(np.uint32)), "the input was changed"
        before = np.full_like(got, SENTINEL)
    touched = np.zeros(got.shape[0], bool)
    outs = np.empty((ns, 2 * n), np.uint32)
    for s in range(ns):
        a = out_shift + s * out_stride
        touched[a:a + n] = True
        outs[s] = got[a:a + n].reshape(-1)
    assert np.array_equal(got[~touched], before[~touched]), "a write outside the streams' outputs"
    gains = None
    if with_gain:
        gg = d_gain.cpu().numpy().view(np.uint32)
        touched = np.zeros(n_gain, bool)
        gains = np.empty((ns, n), np.uint32)
        for s in range(ns):
            touched[s * gain_stride:s * gain_stride + n] = True
            gains[s] = gg[s * gain_stride:s * gain_stride + n]
        assert (gg[~touched] == SENTINEL).all(), "a write outside the streams' gains"
    return outs, gains


def same(got, want, what):
    """got uint32, want float32 (any shape, same size): finite values bit for bit, NaN where the model has NaN"""
    w = np.ascontiguousarray(want).view(np.float32).reshape(-1)
    g = np.ascontiguousarray(got).reshape(-1)
    assert g.size == w.size, what
    nan = np.isnan(w)
    bad = np.where(nan, ~np.isnan(g.view(np.float32)), g != w.view(np.uint32))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {w.size} values differ, the first at {i}: {g[i]:#010x} != {w.view(np.uint32)[i]:#010x}")


def check_call(agc, model, x, what, **kw):
    out, gains = run(agc, x, **kw)
    want_out, want_gains = model.work(x)
    same(out, want_out.view(np.float32), what + ": samples")
    if gains is not None:
        same(gains, want_gains, what + ": gains")
    same(agc.state(model.n_streams).view(np.uint32), model.g, what + ": state")
    return out, gains


@functools.lru_cache(maxsize=None)
def data(seed, ns, n):
    """random complex64 [ns, n] with zeros of both signs and denormals planted in both components"""
    d = np.random.default_rng(seed).normal(size=(ns, n, 2)).astype(np.float32)
    for j, v in enumerate(np.array([0.0, -0.0, 1e-41, -1e-41], np.float32)):
        d[:, (3 + 7 * j) % n, j & 1] = v
    x = d.reshape(ns, 2 * n).view(np.complex64)
    x.setflags(write=False)
    return x


def start_gains(agc, model, ns):
    for s in range(ns):
        g = 0.25 + 0.125 * (s % 13)
        agc.set_gain(s, g)
        model.set_gain(s, g)


# ------------------------------------------------------------------ 1. sizes and streams
@pytest.mark.parametrize("ns", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 3 * T + 5])
def test_sizes_and_streams(n, ns):
    """Strides larger than n (odd ones: the 8-byte path; then multiples of 4: the 16-byte path), every stream its own data and start
    gain, gains asked for and not."""
    agc, model = Agc(0.05, 1.0, 1.0, 65536.0, max_streams=ns, max_samples=n), AM.AgcModel(0.05, 1.0, 1.0, 65536.0, ns)
    assert agc.params() == dict(rate=np.float32(0.05), reference=np.float32(1.0), max_gain=np.float32(65536.0), swap_iq=False, tile=T)
    start_gains(agc, model, ns)
    x = data(n, ns, n)
    check_call(agc, model, x, f"{ns} x {n}, odd strides", in_stride=n + 3, out_stride=n + 5, gain_stride=n + 1)
    check_call(agc, model, x, f"{ns} x {n}, no gains", with_gain=False, in_stride=n + 3, out_stride=n + 5)
    wide = -(-n // 4) * 4
    check_call(agc, model, x, f"{ns} x {n}, aligned rows", in_stride=wide + 4, out_stride=wide + 8, gain_stride=wide + 4)
    check_call(agc, model, x, f"{ns} x {n}, aligned rows, no gains", with_gain=False, in_stride=wide + 4, out_stride=wide + 8)
    agc.close()


@pytest.mark.parametrize("ns", [16384, 16385, 32768, 32769])
def test_batches_at_the_changes_of_streams_per_wavefront(ns):
    """The kernel carries 8 streams per wavefront up to 16384 streams, 16 up to 32768 and 32 beyond."""
    n = T + 3
    agc, model = Agc(0.05, 1.0, 0.5, 65536.0, max_streams=ns, max_samples=n), AM.AgcModel(0.05, 1.0, 0.5, 65536.0, ns)
    agc.set_gain(ns - 1, 3.0)
    model.set_gain(ns - 1, 3.0)
    check_call(agc, model, data(ns, ns, n), f"{ns} x {n}", in_stride=n + 1, out_stride=n + 1, gain_stride=n + 1)
    check_call(agc, model, data(ns, ns, n), f"{ns} x {n}, odd strides", in_stride=n + 2, out_stride=n + 4, gain_stride=n + 2)
    agc.close()


# ------------------------------------------------------------------ 2. amplitudes
def test_input_amplitudes_from_denormal_products_to_overflow():
    """One row per amplitude: 1e-30 (the squares underflow), 2e-20 (the squares are denormal), 1e-3, 1, 1e3, 1e25 (the squares overflow:
    the gain goes to -infinity, and the planted sample with a zero component turns everything behind it into NaN)."""
    amps = np.array([1e-30, 2e-20, 1e-3, 1.0, 1e3, 1e25])
    n = 3 * T + 5
    x = AM.constant_envelope(np.random.default_rng(21), amps.size, n, amps)
    x[5, T + 7] = np.complex64(complex(0.0, 1e25))
    agc, model = Agc(1e-4, 1.0, 1.0, 65536.0, max_streams=amps.size, max_samples=n), AM.AgcModel(1e-4, 1.0, 1.0, 65536.0, amps.size)
    out, gains = check_call(agc, model, x, "amplitudes")
    g = gains.view(np.float32)
    assert np.isinf(g[5, 1:T + 8]).all() and np.isnan(g[5, T + 8:]).all() and np.isfinite(g[:5]).all() and np.isnan(model.g[5])
    m = np.hypot(*out[1].view(np.float32).reshape(-1, 2).astype(np.float64).T)
    assert (m < 1e-18).all() and (m > 0).all()  # the 2e-20 row: its squares are denormal, its outputs are not flushed
    agc.reset()  # the way out of a gain that is not finite
    assert (agc.state() == np.float32(1.0)).all()
    agc.close()


# ------------------------------------------------------------------ 3. the cap
def test_cap_is_reached_inside_the_first_tile_and_held():
    n = 2 * T + 9
    x = AM.constant_envelope(np.random.default_rng(22), 1, n, 1e-3)
    capped, model = Agc(0.5, 1.0, 1.0, 8.0, max_samples=n), AM.AgcModel(0.5, 1.0, 1.0, 8.0)
    _, gains = check_call(capped, model, x, "max_gain 8")
    g = gains.view(np.float32)[0]
    first = int(np.argmax(g == np.float32(8.0)))
    assert 0 < first < T and (g[first:] == np.float32(8.0)).all() and capped.state()[0] == np.float32(8.0)
    free, model = Agc(0.5, 1.0, 1.0, 0.0, max_samples=n), AM.AgcModel(0.5, 1.0, 1.0, 0.0)
    _, gains = check_call(free, model, x, "max_gain 0")
    g = gains.view(np.float32)[0]
    assert (np.diff(g) > 0).all() and g[-1] > 50.0 and free.state()[0] > g[-1]
    capped.close()
    free.close()


# ------------------------------------------------------------------ 4. pieces and cuts
def test_pieces_params_and_reset_at_the_cut():
    n, ns = 3 * T + 5, 3
    x = data(41, ns, n)
    agc = Agc(0.05, 1.0, 0.75, 65536.0, max_streams=ns, max_samples=n)
    whole_out, whole_gains = check_call(agc, AM.AgcModel(0.05, 1.0, 0.75, 65536.0, ns), x, "one call")
    agc.reset()
    rng = np.random.default_rng(42)
    outs, gs, pos, cuts = [], [], 0, [0, T + 3, 1]
    while pos < n:
        c = cuts.pop(0) if cuts else int(rng.integers(0, T + 4))
        c = min(c, n - pos)
        o, g = run(agc, np.ascontiguousarray(x[:, pos:pos + c]), in_stride=c + 2, out_stride=c + 1)
        outs.append(o)
        gs.append(g)
        pos += c
    assert np.array_equal(np.concatenate(outs, axis=1), whole_out) and np.array_equal(np.concatenate(gs, axis=1), whole_gains)
    # set_params between two calls takes effect exactly at the cut
    agc.reset()
    model = AM.AgcModel(0.05, 1.0, 0.75, 65536.0, ns)
    cut = T + 9
    check_call(agc, model, np.ascontiguousarray(x[:, :cut]), "before set_params")
    agc.set_params(0.2, 0.5, 1.5)
    model.set_params(0.2, 0.5, 1.5)
    assert agc.params()["rate"] == np.float32(0.2) and agc.params()["max_gain"] == np.float32(1.5)
    out2, _ = check_call(agc, model, np.ascontiguousarray(x[:, cut:]), "behind set_params")
    assert not np.array_equal(out2, whole_out[:, 2 * cut:])
    # a reset in the middle gives the start gain again
    agc.set_params(0.05, 1.0, 65536.0)
    agc.reset()
    assert (agc.state() == np.float32(0.75)).all()
    out, gains = run(agc, x)
    assert np.array_equal(out, whole_out) and np.array_equal(gains, whole_gains)
    agc.close()


# ------------------------------------------------------------------ 5. in place, alignment, swap_iq
def test_in_place_alignment_and_swap_iq():
    n, ns = 2 * T + 7, 3
    x = data(51, ns, n)
    agc = Agc(0.05, 1.0, 1.0, 65536.0, max_streams=ns, max_samples=n)
    want_out, want_gains = check_call(agc, AM.AgcModel(0.05, 1.0, 1.0, 65536.0, ns), x, "aligned", in_stride=n + 1, out_stride=n + 1, gain_stride=n + 1)
    for kw in (dict(in_place=True, in_stride=n + 1), dict(in_place=True, in_stride=n + 2), dict(in_place=True, in_stride=n + 1, in_shift=1),
               dict(in_shift=1, in_stride=n + 1, out_stride=n + 1), dict(out_shift=1, in_stride=n + 1, out_stride=n + 1),
               dict(in_shift=1, out_shift=1, in_stride=n + 1, out_stride=n + 1), dict(in_stride=n + 1, out_stride=n + 1, gain_stride=n + 2)):
        agc.reset()
        out, gains = run(agc, x, **kw)
        assert np.array_equal(out, want_out) and np.array_equal(gains, want_gains), kw
    agc.reset()
    agc.set_swap_iq(True)
    assert agc.params()["swap_iq"]
    swapped = np.ascontiguousarray(x.view(np.float32).reshape(ns, n, 2)[:, :, ::-1]).reshape(ns, 2 * n).view(np.complex64)
    model = AM.AgcModel(0.05, 1.0, 1.0, 65536.0, ns)
    model.swap_iq = True
    out, gains = check_call(agc, model, swapped, "swap_iq", in_stride=n + 1, out_stride=n + 1, gain_stride=n + 1)
    assert np.array_equal(out, want_out) and np.array_equal(gains, want_gains)  # the bits of the swapped input without swap_iq
    agc.close()


# ------------------------------------------------------------------ 6. the host entry
def test_host_entry_equals_the_device_entry():
    a, b = Agc(0.05, 1.0, 2.0, 65536.0, max_samples=3 * T + 30), Agc(0.05, 1.0, 2.0, 65536.0, max_samples=3 * T + 30)
    model = AM.AgcModel(0.05, 1.0, 2.0, 65536.0)
    for n in (3 * T + 30, 3, 0, 50):
        x = data(60 + n, 1, max(n, 1))[:, :n]
        out, gain = a.work(np.ascontiguousarray(x[0]))
        want_out, want_gain = model.work(x)
        assert out.dtype == np.complex64 and out.size == n and gain.dtype == np.float32 and gain.size == n
        same(out.view(np.uint32), want_out.view(np.float32), f"host entry, {n} samples")
        same(gain.view(np.uint32), want_gain, f"host entry, {n} gains")
        if n:
            d_out, d_gain = run(b, np.ascontiguousarray(x))
            assert np.array_equal(d_out[0], out.view(np.uint32)) and np.array_equal(d_gain[0], gain.view(np.uint32))
        assert np.array_equal(a.state().view(np.uint32), b.state().view(np.uint32))
    two_in, two_out = np.ones(4, np.float32), np.zeros(4, np.float32)
    assert capi.lib.dvbs2_agc_work(a._h, two_in.ctypes.data, 2, two_out.ctypes.data, None) == capi.OK and two_out.all()  # gain is nullable
    a.close()
    b.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_gains_and_output_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    create = lib.dvbs2_agc_create
    refused(capi.EINVAL, "rate must be finite and not negative", create, C.byref(h), -1e-5, 1.0, 1.0, 1.0, 1, 16, 0)
    refused(capi.EINVAL, "reference must be finite", create, C.byref(h), 1e-5, float("inf"), 1.0, 1.0, 1, 16, 0)
    refused(capi.EINVAL, "gain must be finite", create, C.byref(h), 1e-5, 1.0, float("nan"), 1.0, 1, 16, 0)
    refused(capi.EINVAL, "max_gain must be finite and not negative (0: no cap)", create, C.byref(h), 1e-5, 1.0, 1.0, -1.0, 1, 16, 0)
    refused(capi.EINVAL, "max_streams out of range (1..65535)", create, C.byref(h), 1e-5, 1.0, 1.0, 1.0, 0, 16, 0)
    refused(capi.EINVAL, "max_streams out of range (1..65535)", create, C.byref(h), 1e-5, 1.0, 1.0, 1.0, 65536, 16, 0)
    refused(capi.EINVAL, "max_samples out of range (1..2^30)", create, C.byref(h), 1e-5, 1.0, 1.0, 1.0, 1, 0, 0)
    refused(capi.EINVAL, "max_samples out of range (1..2^30)", create, C.byref(h), 1e-5, 1.0, 1.0, 1.0, 1, (1 << 30) + 1, 0)
    refused(capi.EINVAL, "null handle pointer", create, None, 1e-5, 1.0, 1.0, 1.0, 1, 16, 0)
    assert not h
    assert create(C.byref(h), 1e-5, 1.0, 1.0, 1.0, 1, 16, 99) < 0 and not h  # no such device

    n, ns = 100, 2
    agc, model = Agc(0.05, 1.0, 1.0, 65536.0, max_streams=ns, max_samples=n), AM.AgcModel(0.05, 1.0, 1.0, 65536.0, ns)
    first, second = data(70, ns, n), data(71, ns, n)
    check_call(agc, model, first, "before the refusals")
    d_in = torch.from_numpy(np.array(second).view(np.float32)).cuda()
    d_out, d_gain = sentinel(2 * (ns * n + PAD)), sentinel(ns * n + PAD)
    st = stream()
    a, o, g = d_in.data_ptr(), d_out.data_ptr(), d_gain.data_ptr()
    entry = lib.dvbs2_agc_work_device
    refused(capi.ESIZE, "n_samples exceeds max_samples", entry, agc._h, a, n, n + 1, 1, o, n, g, n, st)
    refused(capi.ESIZE, "n_streams exceeds max_streams", entry, agc._h, a, n, n, 3, o, n, g, n, st)
    refused(capi.EINVAL, "n_samples is negative", entry, agc._h, a, n, -1, 2, o, n, g, n, st)
    refused(capi.EINVAL, "n_streams is negative", entry, agc._h, a, n, n, -1, o, n, g, n, st)
    refused(capi.EINVAL, "in is null", entry, agc._h, None, n, n, 2, o, n, g, n, st)
    refused(capi.EINVAL, "out is null", entry, agc._h, a, n, n, 2, None, n, g, n, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, agc._h, a + 4, n, n, 2, o, n, g, n, st)
    refused(capi.EINVAL, "in and out must be 8-byte aligned", entry, agc._h, a, n, n, 2, o + 4, n, g, n, st)
    refused(capi.EINVAL, "gain must be 4-byte aligned", entry, agc._h, a, n, n, 2, o, n, g + 2, n, st)
    refused(capi.EINVAL, "in_stride is below n_samples", entry, agc._h, a, n - 1, n, 2, o, n, g, n, st)
    refused(capi.EINVAL, "out_stride is below n_samples", entry, agc._h, a, n, n, 2, o, n - 1, g, n, st)
    refused(capi.EINVAL, "gain_stride is below n_samples", entry, agc._h, a, n, n, 2, o, n, g, n - 1, st)
    refused(capi.EINVAL, "rate must be finite and not negative", lib.dvbs2_agc_set_params, agc._h, float("nan"), 1.0, 1.0)
    refused(capi.EINVAL, "max_gain must be finite and not negative (0: no cap)", lib.dvbs2_agc_set_params, agc._h, 0.05, 1.0, -2.0)
    refused(capi.EINVAL, "stream index out of range", lib.dvbs2_agc_set_gain, agc._h, 2, 1.0)
    refused(capi.EINVAL, "stream index out of range", lib.dvbs2_agc_set_gain, agc._h, -2, 1.0)
    refused(capi.EINVAL, "gain must be finite", lib.dvbs2_agc_set_gain, agc._h, 0, float("inf"))
    gains = np.zeros(4, np.float32)
    refused(capi.EINVAL, "n_streams out of range (1..max_streams)", lib.dvbs2_agc_state, agc._h, gains.ctypes.data, 3)
    refused(capi.EINVAL, "gains is null", lib.dvbs2_agc_state, agc._h, None, 1)
    assert entry(agc._h, None, 0, 0, 2, None, 0, None, 0, st) == capi.OK  # n_samples == 0: a successful call that does nothing
    assert entry(agc._h, a, 0, 0, 2, o, 0, g, 0, st) == capi.OK
    assert agc.params()["rate"] == np.float32(0.05) and agc.params()["max_gain"] == np.float32(65536.0)
    same(agc.state().view(np.uint32), model.g, "gains behind the refusals")
    assert entry(agc._h, a, 0, n, 1, o, 0, g, 0, st) == capi.OK  # one stream: the strides do not matter (the good call, on stream 0)
    torch.cuda.synchronize()
    out, gg = d_out.cpu().numpy().view(np.uint32), d_gain.cpu().numpy().view(np.uint32)
    want_out, want_gain = model.work(second[:1])
    same(out[:2 * n], want_out.view(np.float32), "the one-stream call behind the refusals")
    same(gg[:n], want_gain, "its gains")
    assert (out[2 * n:] == SENTINEL).all() and (gg[n:] == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = np.ascontiguousarray(second[0]), np.zeros(n, np.complex64)
    refused(capi.ESIZE, "n_samples exceeds max_samples", lib.dvbs2_agc_work, agc._h, host_in.ctypes.data, n + 1, host_out.ctypes.data, None)
    refused(capi.EINVAL, "n_samples is negative", lib.dvbs2_agc_work, agc._h, host_in.ctypes.data, -1, host_out.ctypes.data, None)
    refused(capi.EINVAL, "in is null", lib.dvbs2_agc_work, agc._h, None, n, host_out.ctypes.data, None)
    refused(capi.EINVAL, "out is null", lib.dvbs2_agc_work, agc._h, host_in.ctypes.data, n, None, None)
    assert lib.dvbs2_agc_work(agc._h, None, 0, None, None) == capi.OK
    assert (host_out == 0).all()
    # no refusal touched a gain: both streams go on from where the good calls left them
    check_call(agc, model, first, "behind the refusals")
    agc.close()


# ------------------------------------------------------------------ 8. closed loop through the receiver, noise-free
SCALE = 1.0 / 37.0


def test_closed_loop_through_the_receiver():
    import torch
    seq, plsc, lead = L.SEQ6, L.PLSC, 2001
    tx = L.shaped_six_frames(lead, seed=2027)
    st, ns = stream(), tx.ns
    # the reference: the mean magnitude of the shaped samples at full scale, so that the settled gain is 37 and the symbols behind the
    # matched filter come out at the amplitude they were sent with
    reference = float(torch.linalg.vector_norm(tx.d_y[:2 * lead], dim=1).mean().item())
    d_weak = tx.d_y * SCALE
    agc = Agc(rate=0.05, reference=reference, gain=1.0, max_gain=65536.0, max_samples=ns)
    d_gain = torch.zeros(ns, dtype=torch.float32, device="cuda")
    agc.work_device(d_weak.data_ptr(), ns, ns, 1, d_weak.data_ptr(), ns, d_gain.data_ptr(), ns, st)  # in place
    torch.cuda.synchronize()
    settled = d_gain[2 * lead:2 * (lead + tx.lay["out_syms"])].cpu().numpy()
    print(f"closed loop: reference {reference:.4f}, gain behind the lead {settled.min():.2f} .. {settled.max():.2f} (mean {settled.mean():.2f})")
    assert d_gain[0].item() == 1.0 and 30.0 < settled.min() and settled.max() < 45.0
    rx = L.timing_and_frames(d_weak, ns, L.SPS, L.ROLLOFF, 0, tx.n_all, tol=12)
    recs = rx.recs
    behind = recs[recs["sof_index"] >= lead]
    assert rx.state == capi.PLSYNC_LOCKED and behind["plsc"].tolist() == seq  # every frame behind the settled lead is found
    shifts = set((behind["sof_index"] - (lead + tx.lay["out_offset"])).tolist())
    assert len(shifts) == 1 and abs(shifts.pop() - L.RRC_DELAY) <= 12, shifts
    got = L.decode_frames(rx, plsc, L.GOLD, 0.02, first_sof=lead)
    assert len(got.locked) >= 5 and len(got.locked) == sum(1 for r in recs if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == plsc)
    assert np.array_equal(got.msg, tx.sent[got.data_index])  # the encoder's input bytes
    rx.sync.close()
    agc.close()
