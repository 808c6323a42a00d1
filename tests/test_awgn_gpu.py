"""AWGN channel on the device (dvbs2_awgn_*) against the float32 model of tests/awgn_model.py: every output value BIT FOR BIT (uint32
compare; where the model has a NaN the device must have one), into sentinel-filled buffers whose pads and gaps must stay untouched;
then the encoder and the decoding chain of this library in a closed loop around it."""
import ctypes as C
import functools

import numpy as np
import pytest

import awgn_model as M
from dvbs2rx_amd import Awgn, FecChain, FecEncoder, awgn_sigma, capi
from fec_testlib import SENTINEL, sentinel, stream

pytestmark = pytest.mark.gpu

PAD = 64               # sentinel elements in front of the first and behind the last row
T = capi.AWGN_TILE     # samples of a row one workgroup covers
SEED = 0x1F2E3D4C5B6A7988
SIZES = (1, 2, 3, T - 1, T, T + 1, 3 * T + 5)


@functools.lru_cache(maxsize=None)
def data(seed, ns, n):
    """random float32 [ns, n, 2] with zeros of both signs and denormals planted in both components"""
    d = np.random.default_rng(seed).normal(size=(ns, n, 2)).astype(np.float32)
    for j, v in enumerate(np.array([0.0, -0.0, 1e-41, -1e-41], np.float32)):
        d[:, (3 + 7 * j) % n, j & 1] = v
    d.setflags(write=False)
    return d


def row_sigmas(ns):
    """a different value per row, one of them 0"""
    s = (0.25 + 0.125 * np.arange(ns)).astype(np.float32)
    s[min(1, ns - 1)] = 0.0 if ns > 1 else 0.5
    return s


def run(awgn, n, ns, x=None, first_stream=0, first_index=0, sigmas=None, in_stride=None, out_stride=None, in_shift=0, out_shift=0, in_place=False,
        on_stream=None):
    """One work_device call of ns rows of n samples. x: float32 [ns, n, 2] or None (the noise alone). Row r lies at PAD + in_shift +
    r * in_stride complex elements of a 16-byte-aligned input buffer and is written at PAD + out_shift + r * out_stride of a
    16-byte-aligned sentinel buffer (in place: into the input buffer). sigmas: one float32 per row on the device, or None. Returns
    uint32 [ns, n, 2] after checking that everything else in the buffers is still what it was."""
    import torch
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = (in_stride if in_place else max(n, 1)) if out_stride is None else out_stride
    d_in = None
    if x is not None:
        host_in = np.full((PAD + in_shift + ns * in_stride + PAD, 2), np.float32(9.5), np.float32)
        for r in range(ns):
            a = PAD + in_shift + r * in_stride
            host_in[a:a + n] = x[r]
        d_in = torch.from_numpy(host_in).cuda()
    else:
        assert not in_place
    if in_place:
        out_shift = in_shift
    n_out = PAD + out_shift + (ns - 1) * out_stride + n + PAD
    d_out = d_in if in_place else sentinel(2 * n_out)
    d_sig = torch.from_numpy(np.asarray(sigmas, np.float32)).cuda() if sigmas is not None else None
    assert d_out.data_ptr() % 16 == 0 and (d_in is None or d_in.data_ptr() % 16 == 0)
    torch.cuda.synchronize()
    awgn.work_device(d_in.data_ptr() + 8 * (PAD + in_shift) if d_in is not None else 0, in_stride, n, ns, d_out.data_ptr() + 8 * (PAD + out_shift),
                     out_stride, first_stream=first_stream, first_index=first_index, d_sigma=d_sig.data_ptr() if d_sig is not None else 0,
                     stream=stream() if on_stream is None else on_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    if in_place:
        before = host_in.view(np.uint32)
    else:
        if d_in is not None:
            assert np.array_equal(d_in.cpu().numpy().view(np.uint32), host_in.view(np.uint32)), "the input was changed"
        before = np.full_like(got, SENTINEL)
    touched = np.zeros(got.shape[0], bool)
    outs = np.empty((ns, n, 2), np.uint32)
    for r in range(ns):
        a = PAD + out_shift + r * out_stride
        touched[a:a + n] = True
        outs[r] = got[a:a + n]
    assert np.array_equal(got[~touched], before[~touched]), "a write outside the rows' outputs"
    return outs


def same(got, want, what):
    """got uint32, want float32 (same size): finite values bit for bit, NaN where the model has NaN"""
    w = np.ascontiguousarray(want, np.float32).reshape(-1)
    g = np.ascontiguousarray(got).reshape(-1)
    assert g.size == w.size, what
    nan = np.isnan(w)
    bad = np.where(nan, ~np.isnan(g.view(np.float32)), g != w.view(np.uint32))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {w.size} values differ, the first at {i}: {g[i]:#010x} != {w.view(np.uint32)[i]:#010x}")


def check_call(awgn, sigma, n, ns, what, x=None, first_stream=0, first_index=0, sigmas=None, **kw):
    got = run(awgn, n, ns, x=x, first_stream=first_stream, first_index=first_index, sigmas=sigmas, **kw)
    want = M.rows(SEED, first_stream, first_index, n, ns, sigma if sigmas is None else sigmas, x)
    same(got, want, what)
    return got


@pytest.fixture(scope="module")
def awgn():
    a = Awgn(SEED, 0.75, max_streams=65535, max_samples=1 << 16)
    yield a
    a.close()


@pytest.mark.parametrize("per_row", (False, True))
@pytest.mark.parametrize("ns", (1, 2, 3, 65))
def test_sizes_and_rows(awgn, ns, per_row):
    sig = row_sigmas(ns) if per_row else None
    for n in SIZES:
        x = data(1, ns, n)
        even, odd = (n + 3) & ~1, (n + 2) | 1  # even strides keep every row on the 16-byte path, odd ones put every other row off it
        check_call(awgn, 0.75, n, ns, f"n {n}, even strides", x=x, sigmas=sig, in_stride=even, out_stride=even + 2)
        check_call(awgn, 0.75, n, ns, f"n {n}, odd strides", x=x, sigmas=sig, in_stride=odd, out_stride=odd + 2)


def test_65535_rows_of_three():
    a = Awgn(SEED, 0.5, max_streams=65535, max_samples=4)
    x = data(2, 65535, 3)
    check_call(a, 0.5, 3, 65535, "65535 rows", x=x, first_stream=(1 << 32) - 9, first_index=1)
    a.close()


@pytest.mark.parametrize("first_stream", (0, (1 << 32) - 1, (1 << 64) - 2))
@pytest.mark.parametrize("first_index", (0, 1, (1 << 33) - 1, 1 << 33, (1 << 40) + 1))
def test_position(awgn, first_index, first_stream):
    """3 rows, so the last first_stream wraps inside the call; odd and even starts with odd and even lengths: the half blocks."""
    for n in (4, 5, T + 1, T + 2):
        for start in (first_index, first_index + 1):
            check_call(awgn, 0.75, n, 3, f"n {n} from {start}", x=data(3, 3, n), first_stream=first_stream, first_index=start, in_stride=n + 4,
                       out_stride=n + 6)
    check_call(awgn, 0.75, 7, 1, "the last indices", x=data(3, 1, 7), first_stream=first_stream, first_index=(1 << 63) - 1 - 7)


def test_pieces_equal_one_call(awgn):
    """No state links two calls: a row cut anywhere, the pieces issued on two HIP streams with advancing first_index, has the bits of
    one call; so have the rows of a call issued one by one."""
    import torch
    n, first = 3 * T + 5, (1 << 33) - T - 3
    x = data(4, 1, n)
    whole = check_call(awgn, 0.75, n, 1, "one call", x=x, first_stream=12, first_index=first)
    rng = np.random.default_rng(5)
    cuts = [1, 2, T - 1, T, T + 1, int(rng.integers(1, n // 2)) * 2 + 1, int(rng.integers(1, n // 2)) * 2]
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_in = torch.from_numpy(np.array(x[0])).cuda()
    for cut in cuts:
        d_out = sentinel(2 * (n + PAD))
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(((0, cut), (cut, n))):
            awgn.work_device(d_in.data_ptr() + 8 * a, n, b - a, 1, d_out.data_ptr() + 8 * a, n, first_stream=12, first_index=first + a,
                             stream=side[k].cuda_stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:2 * n], whole.reshape(-1)), f"cut at {cut}"
        assert (got[2 * n:] == SENTINEL).all()
    # the running position of the Python class: the same pieces without naming first_index
    awgn.position = first
    d_out = sentinel(2 * (n + PAD))
    for a, b in ((0, T + 1), (T + 1, n)):
        awgn.work_device(d_in.data_ptr() + 8 * a, n, b - a, 1, d_out.data_ptr() + 8 * a, n, first_stream=12, stream=stream())
    torch.cuda.synchronize()
    assert awgn.position == first + n and np.array_equal(d_out.cpu().numpy().view(np.uint32)[:2 * n], whole.reshape(-1))
    # rows one by one
    x4 = data(6, 4, T + 3)
    four = check_call(awgn, 0.75, T + 3, 4, "four rows", x=x4, first_stream=(1 << 64) - 2, first_index=5)
    for r in range(4):
        one = check_call(awgn, 0.75, T + 3, 1, f"row {r} alone", x=x4[r:r + 1], first_stream=((1 << 64) - 2 + r) & M.U64, first_index=5)
        assert np.array_equal(one[0], four[r])


def test_in_place_alignment_noise_only_and_special_values(awgn):
    n, ns = 2 * T + 3, 3
    x = data(7, ns, n)
    for first in (0, 1):
        ref = check_call(awgn, 0.75, n, ns, "out of place", x=x, first_index=first, in_stride=n + 1, out_stride=n + 3)
        got = check_call(awgn, 0.75, n, ns, "in place", x=x, first_index=first, in_stride=n + 1, in_place=True)
        assert np.array_equal(got, ref)
        # rows shifted by one complex element: the other parity of 16-byte alignment, input and output alike and each alone
        for in_shift, out_shift in ((1, 1), (1, 0), (0, 1)):
            got = check_call(awgn, 0.75, n, ns, f"shifted {in_shift} {out_shift}", x=x, first_index=first, in_stride=n + 1, out_stride=n + 3,
                             in_shift=in_shift, out_shift=out_shift)
            assert np.array_equal(got, ref)
        got = check_call(awgn, 0.75, n, ns, "in place, shifted", x=x, first_index=first, in_stride=n + 1, in_shift=1, in_place=True)
        assert np.array_equal(got, ref)
        # the noise alone: the product, on both paths
        alone = check_call(awgn, 0.75, n, ns, "noise only", first_index=first, out_stride=n + 3)
        assert np.array_equal(check_call(awgn, 0.75, n, ns, "noise only, shifted", first_index=first, out_stride=n + 3, out_shift=1), alone)
        same(alone, M.rows(SEED, 0, first, n, ns, np.float32(0.75)), "the product alone")
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-41, -1e-41, 1e-45, 3.4e38, -3.4e38, 1.0, -1.0], np.float32)
    xs = np.stack([np.resize(special, 2 * 48).reshape(48, 2), np.resize(special[::-1], 2 * 48).reshape(48, 2)])
    for sig in (None, np.array([0.0, np.inf], np.float32), np.array([-1.5, np.nan], np.float32), np.array([1e-40, 3e38], np.float32)):
        check_call(awgn, 0.75, 48, 2, f"special values, sigmas {sig}", x=xs, sigmas=sig)
    got = check_call(awgn, 0.75, 48, 2, "sigma 0", x=xs, sigmas=np.zeros(2, np.float32)).view(np.float32)
    keep = ~np.isnan(xs) & (xs != 0)
    assert np.array_equal(got[keep], xs[keep]) and (got[xs == 0] == 0).all()  # sigma == 0 returns the input; a -0 may come out +0


def test_corner_words_on_the_device():
    a = Awgn(M.CORNER_SEED, 1.0, max_streams=1, max_samples=2)
    for idx in M.corner_indices():
        for n in (1, 2):
            want = M.noise(M.CORNER_SEED, M.CORNER_STREAM, idx + np.arange(n))  # sigma 1: the product is the noise itself
            same(run(a, n, 1, first_stream=M.CORNER_STREAM, first_index=idx), want, f"index {idx}, {n} samples")
            x = data(8, 1, n)
            same(run(a, n, 1, x=x, first_stream=M.CORNER_STREAM, first_index=idx), x[0] + want, f"index {idx}, {n} samples on an input")
    a.close()


def test_host_entry_equals_device_entry_and_setters_hold():
    a = Awgn(SEED, 0.75, max_streams=4, max_samples=4 * T)
    assert a.params() == dict(seed=SEED, sigma=np.float32(0.75), max_streams=4, max_samples=4 * T)
    n = 2 * T + 1
    x = data(9, 1, n)
    xc = np.ascontiguousarray(x[0]).view(np.complex64).reshape(-1)
    dev = check_call(a, 0.75, n, 1, "device entry", x=x, first_stream=3, first_index=77)
    host = a.work(xc, stream_id=3, first_index=77)
    assert np.array_equal(host.view(np.uint32), dev.reshape(-1))
    same(a.work(n, stream_id=3, first_index=78).view(np.uint32), M.rows(SEED, 3, 78, n, 1, np.float32(0.75)), "host entry, noise only")
    a.position = 10
    first = a.work(xc[:5], stream_id=3)
    second = a.work(xc[5:9], stream_id=3)
    assert a.position == 19
    same(np.concatenate([first, second]).view(np.uint32), M.rows(SEED, 3, 10, 9, 1, np.float32(0.75), x[:, :9]), "host entry, running position")
    a.set_sigma(0.125)
    a.set_seed(SEED + 1)
    assert a.params()["sigma"] == np.float32(0.125) and a.params()["seed"] == SEED + 1
    got = run(a, n, 1, x=x, first_stream=3, first_index=77)
    same(got, M.rows(SEED + 1, 3, 77, n, 1, np.float32(0.125), x), "after set_sigma and set_seed")
    assert np.array_equal(a.work(xc, stream_id=3, first_index=77).view(np.uint32), got.reshape(-1))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(capi.Dvbs2Error) as e:
            a.set_sigma(bad)
        assert e.value.code == capi.EINVAL and "sigma" in str(e.value)
    assert a.params()["sigma"] == np.float32(0.125)
    a.close()


def test_refusals_leave_the_output_untouched():
    import torch
    a = Awgn(SEED, 1.0, max_streams=4, max_samples=64)
    d_in = torch.zeros(2 * 1024, dtype=torch.float32, device="cuda")
    d_out = sentinel(2 * 1024)
    d_sig = torch.ones(8, dtype=torch.float32, device="cuda")
    i, o, s = d_in.data_ptr(), d_out.data_ptr(), d_sig.data_ptr()
    big = (1 << 63) - 1
    #        d_in in_stride n ns first_stream first_index d_sigma d_out out_stride   code   the text names
    rows = [(i, 64, -1, 1, 0, 0, 0, o, 64, capi.EINVAL, "n_samples"),
            (i, 64, 8, -1, 0, 0, 0, o, 64, capi.EINVAL, "n_streams"),
            (i, 64, 65, 1, 0, 0, 0, o, 64, capi.ESIZE, "n_samples"),
            (i, 64, 8, 5, 0, 0, 0, o, 64, capi.ESIZE, "n_streams"),
            (i, 64, 8, 1, 0, -1, 0, o, 64, capi.EINVAL, "first_index"),
            (i, 64, 8, 1, 0, big - 7, 0, o, 64, capi.EINVAL, "first_index"),
            (i, 64, 8, 1, 0, 0, 0, 0, 64, capi.EINVAL, "out"),
            (i + 4, 64, 8, 1, 0, 0, 0, o, 64, capi.EINVAL, "in and out"),
            (i, 64, 8, 1, 0, 0, 0, o + 4, 64, capi.EINVAL, "in and out"),
            (i, 64, 8, 1, 0, 0, s + 2, o, 64, capi.EINVAL, "sigma"),
            (i, 7, 8, 2, 0, 0, 0, o, 64, capi.EINVAL, "in_stride"),
            (i, 64, 8, 2, 0, 0, 0, o, 7, capi.EINVAL, "out_stride")]
    for *args, code, name in rows:
        rc = capi.lib.dvbs2_awgn_add_device(a._h, args[0] or None, args[1], args[2], args[3], args[4], args[5], args[6] or None, args[7] or None,
                                            args[8], stream() or None)
        assert rc == code and name in capi.lib.dvbs2_last_error().decode(), (args, rc, capi.lib.dvbs2_last_error())
    # accepted: nothing to do, the largest first_index, strides that do not matter with one row
    for n, ns, first in ((0, 1, 0), (8, 0, 0), (0, 0, big), (8, 1, big - 8)):
        assert capi.lib.dvbs2_awgn_add_device(a._h, i, 1, n, ns, 0, first, None, o + 8 * 512, 1, stream() or None) == capi.OK
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    assert (got[:1024] == SENTINEL).all() and (got[1024 + 16:] == SENTINEL).all() and (got[1024:1024 + 16] != SENTINEL).all()
    # the host entry
    out = np.full(16, np.float32(5.0), np.float32)
    x = np.zeros(16, np.float32)
    for n, first, src, dst, code, name in ((-1, 0, x, out, capi.EINVAL, "n_samples"), (65, 0, x, out, capi.ESIZE, "n_samples"),
                                           (8, -1, x, out, capi.EINVAL, "first_index"), (8, big - 7, x, out, capi.EINVAL, "first_index"),
                                           (8, 0, x, None, capi.EINVAL, "out")):
        rc = capi.lib.dvbs2_awgn_add(a._h, src.ctypes.data, n, 0, first, dst.ctypes.data if dst is not None else None)
        assert rc == code and name in capi.lib.dvbs2_last_error().decode(), (n, first, rc)
    assert (out == 5.0).all()
    assert capi.lib.dvbs2_awgn_add(a._h, None, 0, 0, 0, None) == capi.OK
    for args in ((np.nan, 1, 1), (1.0, 0, 1), (1.0, 1, 0)):
        h = C.c_void_p()
        assert capi.lib.dvbs2_awgn_create(C.byref(h), 1, *args, 0) == capi.EINVAL and not h
    a.close()


def test_closed_loop_qpsk_1_4_short():
    """FecEncoder (scrambler on) -> Awgn in place on the XFECFRAME symbols, one row per frame -> FecChain (descrambler on). At Es/N0 =
    1 dB, more than 3 dB above the MODCOD's ideal threshold of -2.35 dB (EN 302 307-1 table 13), every frame decodes; at -8 dB, far
    below it, at least one does not: the noise reaches the decoder."""
    import torch
    nf = 8
    enc = FecEncoder(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, max_frames=nf)
    enc.set_scramble(True)
    chain = FecChain(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, group_size=4, max_frames=nf, max_trials=25)
    chain.set_descramble(True)
    msg = np.random.default_rng(11).integers(0, 256, (nf, enc.in_bytes), dtype=np.uint8)
    clean = enc.work(msg, want=["syms"])["syms"]
    ns = enc.n_syms
    assert nf * ns * 2 == 129600
    failed = {}
    for esn0 in (1.0, -8.0):
        sigma = awgn_sigma(esn0_db=esn0, es=1, sps=1)
        a = Awgn(SEED, sigma, max_streams=nf, max_samples=ns)
        d = torch.from_numpy(clean.view(np.float32).reshape(nf, 2 * ns).copy()).cuda()
        a.work_device(d.data_ptr(), ns, ns, nf, d.data_ptr(), ns, first_stream=100, first_index=0, stream=stream())
        torch.cuda.synchronize()
        rx = d.cpu().numpy()
        diff = (rx.astype(np.float64) - clean.view(np.float32).reshape(nf, 2 * ns)).reshape(-1)
        s2 = float(diff.var(ddof=1))
        assert abs(s2 / float(sigma) ** 2 - 1) <= 5 * np.sqrt(2 / 129600), (esn0, s2, sigma)
        out, ret, corr = chain.work(rx.view(np.complex64), np.float32(2 * float(sigma) ** 2))
        failed[esn0] = int((out != msg).any(axis=1).sum())
        if esn0 > 0:
            assert (ret >= 0).all() and np.array_equal(out, msg)
        a.close()
    assert failed[1.0] == 0 and failed[-8.0] >= 1
    enc.close()
    chain.close()
