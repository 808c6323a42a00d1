"""IQ sample converter on the device (dvbs2_iqconv_*) against the model of tests/iqconv_model.py: every float BIT FOR BIT (uint32
compare), every code and every statistic equal, into sentinel-filled buffers whose pads and gaps must stay untouched; then the transmit
and the receive side of this library in a closed loop through a u8 and an s16 stream."""
import ctypes as C
import functools

import numpy as np
import pytest

import iqconv_model as M
import loopback as L
from dvbs2rx_amd import Agc, IqConverter, capi
from fec_testlib import SENTINEL, sentinel, stream

pytestmark = pytest.mark.gpu

CODE_FILL = 0xA5       # what the code buffers hold outside the rows
PAD = 64               # sentinel elements (floats: complex elements, codes: bytes, statistics: words) around the rows
T = capi.IQCONV_TILE   # samples of a row one workgroup covers
SIZES = (1, 2, 3, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5)
STATS_START = 1000     # what the statistics words hold before a call: a call adds


def width(fmt):
    return np.dtype(M.DTYPE[fmt]).itemsize


@functools.lru_cache(maxsize=None)
def codes_of(fmt, seed, ns, n):
    """random codes [ns, n, 2] with both rails planted"""
    c = np.random.default_rng(seed).integers(M.LO[fmt], M.HI[fmt] + 1, (ns, n, 2)).astype(M.DTYPE[fmt])
    c[:, 0, 0] = M.LO[fmt]
    c[:, n // 2, 1] = M.HI[fmt]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def floats_of(seed, ns, n):
    """random float32 [ns, n, 2]: most inside full scale, some beyond, zeros of both signs, a NaN and an infinity planted"""
    x = (np.random.default_rng(seed).normal(size=(ns, n, 2)) * 0.45).astype(np.float32)
    for j, v in enumerate(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-41, 3.0, -3.0], np.float32)):
        x[:, (2 + 5 * j) % n, j & 1] = v
    x.setflags(write=False)
    return x


class Stats:
    """n_streams x 3 uint64 on the device between sentinel words, each counter starting at STATS_START + its index"""

    def __init__(self, ns):
        import torch
        host = np.full(PAD + 3 * ns + PAD, SENTINEL, np.uint64)
        self.start = STATS_START + np.arange(3 * ns, dtype=np.uint64)
        host[PAD:PAD + 3 * ns] = self.start
        self.ns, self.buf = ns, torch.from_numpy(host.view(np.int64)).cuda()
        self.ptr = self.buf.data_ptr() + 8 * PAD

    def read(self):
        """[[samples, clipped, energy] per row] added since the start (mod 2^64), after checking the pads"""
        got = self.buf.cpu().numpy().view(np.uint64)
        assert (got[:PAD] == SENTINEL).all() and (got[PAD + 3 * self.ns:] == SENTINEL).all(), "a write outside the statistics"
        added = got[PAD:PAD + 3 * self.ns] - self.start  # uint64: wraps as the counters do
        return [[int(v) for v in added[3 * r:3 * r + 3]] for r in range(self.ns)]


def place_codes(fmt, codes, stride, shift):
    """codes [ns, n, 2] into a byte buffer: row r at PAD + shift + r * stride * bytes-per-sample. Returns (host bytes, device tensor)."""
    import torch
    ns, n = codes.shape[:2]
    bps = 2 * width(fmt)
    host = np.full(PAD + shift + ((ns - 1) * stride + n) * bps + PAD, CODE_FILL, np.uint8)
    for r in range(ns):
        a = PAD + shift + r * stride * bps
        host[a:a + n * bps] = np.ascontiguousarray(codes[r]).reshape(-1).view(np.uint8)
    return host, torch.from_numpy(host).cuda()


def unpack(conv, codes, in_stride=None, out_stride=None, code_shift=0, float_shift=0, stats=True, on_stream=None, into=None):
    """One unpack_device call on codes [ns, n, 2]; float_shift in complex elements (0 or 1: 16-byte aligned or not). Returns (uint32
    [ns, n, 2], statistics per row or None) after checking that everything else in the buffers is what it was."""
    import torch
    fmt = conv.format
    ns, n = codes.shape[:2]
    in_stride = n if in_stride is None else in_stride
    out_stride = n if out_stride is None else out_stride
    host_in, d_in = place_codes(fmt, codes, in_stride, code_shift)
    n_out = PAD + float_shift + (ns - 1) * out_stride + n + PAD
    d_out = sentinel(2 * n_out)
    st = (into or Stats(ns)) if stats else None
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    conv.unpack_device(d_in.data_ptr() + PAD + code_shift, in_stride, n, ns, d_out.data_ptr() + 8 * (PAD + float_shift), out_stride,
                       d_stats=st.ptr if st else 0, stream=stream() if on_stream is None else on_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy(), host_in), "the input was changed"
    got = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    touched = np.zeros(got.shape[0], bool)
    outs = np.empty((ns, n, 2), np.uint32)
    for r in range(ns):
        a = PAD + float_shift + r * out_stride
        touched[a:a + n] = True
        outs[r] = got[a:a + n]
    assert (got[~touched] == SENTINEL).all(), "a write outside the rows' outputs"
    return outs, (st.read() if st and into is None else None)


def pack(conv, x, in_stride=None, out_stride=None, code_shift=0, float_shift=0, stats=True, on_stream=None, into=None):
    """One pack_device call on float32 x [ns, n, 2]. Returns (codes [ns, n, 2], statistics per row or None), the rest checked."""
    import torch
    fmt = conv.format
    ns, n = x.shape[:2]
    bps = 2 * width(fmt)
    in_stride = n if in_stride is None else in_stride
    out_stride = n if out_stride is None else out_stride
    host_in = np.full((PAD + float_shift + (ns - 1) * in_stride + n + PAD, 2), np.float32(9.5), np.float32)
    for r in range(ns):
        a = PAD + float_shift + r * in_stride
        host_in[a:a + n] = x[r]
    d_in = torch.from_numpy(host_in).cuda()
    n_bytes = PAD + code_shift + ((ns - 1) * out_stride + n) * bps + PAD
    d_out = torch.full((n_bytes,), CODE_FILL, dtype=torch.uint8, device="cuda")
    st = (into or Stats(ns)) if stats else None
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    conv.pack_device(d_in.data_ptr() + 8 * (PAD + float_shift), in_stride, n, ns, d_out.data_ptr() + PAD + code_shift, out_stride,
                     d_stats=st.ptr if st else 0, stream=stream() if on_stream is None else on_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), host_in.view(np.uint32)), "the input was changed"
    got = d_out.cpu().numpy()
    touched = np.zeros(n_bytes, bool)
    outs = np.empty((ns, n, 2), M.DTYPE[fmt])
    for r in range(ns):
        a = PAD + code_shift + r * out_stride * bps
        touched[a:a + n * bps] = True
        outs[r] = got[a:a + n * bps].view(M.DTYPE[fmt]).reshape(n, 2)
    assert (got[~touched] == CODE_FILL).all(), "a write outside the rows' outputs"
    return outs, (st.read() if st and into is None else None)


def check_unpack(conv, gain, codes, what, **kw):
    got, st = unpack(conv, codes, **kw)
    want, want_st = M.unpack_rows(conv.format, gain, codes)
    bad = got != want.view(np.uint32)
    assert not bad.any(), f"unpack, {what}: {int(bad.sum())} of {bad.size} values differ, the first at {np.argwhere(bad)[0].tolist()}"
    if st is not None:
        assert st == want_st, f"unpack, {what}: statistics"
    return got


def check_pack(conv, gain, x, what, **kw):
    got, st = pack(conv, x, **kw)
    want, want_st = M.pack_rows(conv.format, gain, x)
    bad = got != want
    assert not bad.any(), f"pack, {what}: {int(bad.sum())} of {bad.size} codes differ, the first at {np.argwhere(bad)[0].tolist()}"
    if st is not None:
        assert st == want_st, f"pack, {what}: statistics"
    return got


@pytest.fixture(scope="module")
def convs():
    made = {fmt: IqConverter(M.NAMES[fmt], 0.75, max_streams=65535, max_samples=1 << 16) for fmt in M.FORMATS}
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("ns", (1, 2, 3, 64, 65))
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_sizes_and_rows(convs, fmt, ns):
    conv = convs[fmt]
    for n in SIZES:
        c, x = codes_of(fmt, 1, ns, n), floats_of(2, ns, n)
        for in_stride, out_stride, what in ((n, n, "dense"), (n + 1 + (n & 1), n + 3 + (n & 1), "odd strides")):
            check_unpack(conv, 0.75, c, f"n {n}, {ns} rows, {what}", in_stride=in_stride, out_stride=out_stride, stats=n % 2 == 1)
            check_pack(conv, 0.75, x, f"n {n}, {ns} rows, {what}", in_stride=in_stride, out_stride=out_stride, stats=n % 2 == 1)


@pytest.mark.parametrize("rows", (1, 3))
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_alignment(convs, fmt, rows):
    """Every byte phase of the code buffer against both phases of the float buffer: the wide path at (0, 0) with an even stride, the edge
    path everywhere else, its head and tail at every phase. Three rows with an odd stride change the phase from row to row."""
    conv = convs[fmt]
    for n in (5, 302, T + 11):
        c, x = codes_of(fmt, 3, rows, n), floats_of(4, rows, n)
        ref_u = check_unpack(conv, 0.75, c, f"n {n}, aligned")
        ref_p = check_pack(conv, 0.75, x, f"n {n}, aligned")
        stride = n + 1 + (n & 1) if rows > 1 else n  # odd
        for code_shift in range(0, 16, width(fmt)):
            for float_shift in (0, 1):
                what = f"n {n}, codes + {code_shift} bytes, floats + {8 * float_shift} bytes"
                got = check_unpack(conv, 0.75, c, what, in_stride=stride, out_stride=stride + 2, code_shift=code_shift, float_shift=float_shift)
                assert np.array_equal(got, ref_u)
                got = check_pack(conv, 0.75, x, what, in_stride=stride + 2, out_stride=stride, code_shift=code_shift, float_shift=float_shift)
                assert np.array_equal(got, ref_p)


@pytest.mark.parametrize("gain", (1.0, 0.3, 16.0))
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_every_code_and_the_edge_vector(fmt, gain):
    every = M.all_codes(fmt).reshape(1, -1, 2)
    conv = IqConverter(fmt, gain, max_streams=2, max_samples=every.shape[1])
    check_unpack(conv, gain, every, "every code")
    check_unpack(conv, gain, every[:, ::-1], "every code, on the edge path", code_shift=width(fmt), float_shift=1)
    edge = M.edge_values(fmt).reshape(1, -1, 2)
    check_pack(conv, gain, edge, "the edge vector")
    check_pack(conv, gain, edge, "the edge vector, on the edge path", code_shift=width(fmt), float_shift=1)
    two = np.concatenate([edge, edge[:, ::-1]])
    check_pack(conv, gain, two, "the edge vector, two rows", in_stride=edge.shape[1] + 1, out_stride=edge.shape[1] + 1)
    conv.close()


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_pieces_equal_one_call(convs, fmt):
    """No state links two calls: a row cut into calls that start at odd addresses has the bits, the codes and the statistics of one call."""
    import torch
    conv = convs[fmt]
    n, bps = 3 * T + 11, 2 * width(fmt)
    cuts = [0, 1, T - 3, T + 2, n]
    c, x = codes_of(fmt, 5, 1, n), floats_of(6, 1, n)
    whole_u, st_u = unpack(conv, c)
    whole_p, st_p = pack(conv, x)
    assert st_u == M.unpack_rows(fmt, 0.75, c)[1] and st_p == M.pack_rows(fmt, 0.75, x)[1]
    d_codes = torch.from_numpy(np.ascontiguousarray(c[0]).reshape(-1).view(np.uint8).copy()).cuda()
    d_floats = sentinel(2 * (n + PAD))
    st = Stats(1)
    for a, b in zip(cuts, cuts[1:]):
        conv.unpack_device(d_codes.data_ptr() + a * bps, n, b - a, 1, d_floats.data_ptr() + 8 * a, n, d_stats=st.ptr, stream=stream())
    torch.cuda.synchronize()
    got = d_floats.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:2 * n], whole_u.reshape(-1)) and (got[2 * n:] == SENTINEL).all() and st.read() == st_u
    d_x = torch.from_numpy(np.array(x[0])).cuda()
    d_out = torch.full((n * bps + PAD,), CODE_FILL, dtype=torch.uint8, device="cuda")
    st = Stats(1)
    for a, b in zip(cuts, cuts[1:]):
        conv.pack_device(d_x.data_ptr() + 8 * a, n, b - a, 1, d_out.data_ptr() + a * bps, n, d_stats=st.ptr, stream=stream())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:n * bps].view(M.DTYPE[fmt]), whole_p.reshape(-1)) and (got[n * bps:] == CODE_FILL).all() and st.read() == st_p


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_statistics(convs, fmt):
    import torch
    conv = convs[fmt]
    # a row with known rails: three components on a rail among the middle code
    n = T + 9
    known = np.full((2, n, 2), M.MID[fmt], M.DTYPE[fmt])
    known[0, 0, 0], known[0, T, 1], known[0, n - 1, 1], known[1, 5, 0] = M.LO[fmt], M.HI[fmt], M.HI[fmt], M.LO[fmt]
    _, st = unpack(conv, known, in_stride=n + 1, out_stride=n + 1)
    d = [int(M.level(fmt, np.array(v, M.DTYPE[fmt]))) for v in (M.MID[fmt], M.LO[fmt], M.HI[fmt])]
    assert st == [[n, 3, (2 * n - 3) * d[0] ** 2 + d[1] ** 2 + 2 * d[2] ** 2], [n, 1, (2 * n - 1) * d[0] ** 2 + d[1] ** 2]]
    # pack: one value far outside, one that rounds onto the rail, one NaN, in a row of zeros
    x = np.zeros((1, n, 2), np.float32)
    full, bias = float(M.FULL[fmt]), float(M.BIAS[fmt])
    x[0, 1, 0], x[0, T + 1, 1], x[0, n - 1, 0] = 7.0, (M.HI[fmt] + 0.25 - bias) / full, np.nan
    unit = IqConverter(fmt, 1.0, max_samples=n)
    got, st = pack(unit, x)
    want, want_st = M.pack_rows(fmt, 1.0, x)
    assert np.array_equal(got, want) and st == want_st and st[0][:2] == [n, 2] and got[0, T + 1, 1] == M.HI[fmt]
    unit.close()
    # without statistics nothing is reduced and nothing is written: a sentinel buffer of the statistics' size stays as it is
    idle = Stats(3)
    c3, x3 = codes_of(fmt, 7, 3, n), floats_of(8, 3, n)
    check_unpack(conv, 0.75, c3, "without statistics", stats=False)
    check_pack(conv, 0.75, x3, "without statistics", stats=False)
    assert idle.read() == [[0, 0, 0]] * 3
    # two calls on two HIP streams add into the same statistics
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    shared = Stats(3)
    unpack(conv, c3, on_stream=side[0].cuda_stream, into=shared)
    pack(conv, x3, on_stream=side[1].cuda_stream, into=shared)
    a, b = M.unpack_rows(fmt, 0.75, c3)[1], M.pack_rows(fmt, 0.75, x3)[1]
    assert shared.read() == [[p + q for p, q in zip(ra, rb)] for ra, rb in zip(a, b)]
    d_c = place_codes(fmt, c3, n, 0)[1]
    d_f = torch.zeros(3 * n * 2, dtype=torch.float32, device="cuda")
    shared = Stats(3)
    torch.cuda.synchronize()
    for s in side:  # enqueued back to back, no synchronisation between them
        conv.unpack_device(d_c.data_ptr() + PAD, n, n, 3, d_f.data_ptr(), n, d_stats=shared.ptr, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert shared.read() == [[2 * v for v in row] for row in a]


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_host_entries_equal_the_device_entries(fmt):
    import torch
    top = T + 3
    conv = IqConverter(fmt, 0.3, max_streams=1, max_samples=top)
    assert conv.params() == dict(format=fmt, gain=np.float32(0.3), max_streams=1, max_samples=top, tile=T)
    for n in (1, 65, top):
        c, x = codes_of(fmt, 9, 1, n), floats_of(10, 1, n)
        dev_u, st_u = unpack(conv, c)
        d_out = sentinel(2 * (n + PAD))
        st = conv.unpack_to_device(np.array(c[0]), d_out.data_ptr(), stats=True)
        got = d_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:2 * n], dev_u.reshape(-1)) and (got[2 * n:] == SENTINEL).all()
        assert [st["samples"], st["clipped"], st["energy"]] == st_u[0]
        assert conv.unpack_to_device(np.array(c[0]), d_out.data_ptr()) is None
        dev_p, st_p = pack(conv, x)
        d_x = torch.from_numpy(np.array(x[0])).cuda()
        codes, st = conv.pack_from_device(d_x.data_ptr(), n, stats=True)
        assert np.array_equal(codes, dev_p[0]) and [st["samples"], st["clipped"], st["energy"]] == st_p[0]
        assert np.array_equal(conv.pack_from_device(d_x.data_ptr(), n), dev_p[0])
    # the host words are added to, and the gain holds for the calls after set_gain
    words = np.array([1, 2, 3], np.uint64)
    c = codes_of(fmt, 9, 1, 65)
    assert capi.lib.dvbs2_iqconv_unpack_to_device(conv._h, np.array(c[0]).ctypes.data, 65, d_out.data_ptr(), words.ctypes.data) == capi.OK
    want = M.unpack_rows(fmt, 0.3, c)[1][0]
    assert [int(v) for v in words] == [1 + want[0], 2 + want[1], 3 + want[2]]
    conv.set_gain(16.0)
    assert conv.params()["gain"] == np.float32(16.0)
    check_unpack(conv, 16.0, c, "after set_gain")
    check_pack(conv, 16.0, floats_of(10, 1, 65), "after set_gain")
    for bad in (0.0, -1.0, np.nan, np.inf, 2.0 ** 65):
        with pytest.raises(capi.Dvbs2Error) as e:
            conv.set_gain(bad)
        assert e.value.code == capi.EINVAL and "gain" in str(e.value)
    assert conv.params()["gain"] == np.float32(16.0)
    conv.close()


def test_refusals_leave_output_and_statistics_untouched():
    import torch
    lib = capi.lib
    for fmt in (M.U8, M.S16):
        conv = IqConverter(fmt, 1.0, max_streams=4, max_samples=64)
        d_codes = torch.full((4096,), CODE_FILL, dtype=torch.uint8, device="cuda")
        d_floats = sentinel(4096)
        st = Stats(4)
        c, f, s = d_codes.data_ptr(), d_floats.data_ptr(), st.ptr
        for entry, first, second, names in ((lib.dvbs2_iqconv_unpack_device, c, f, ("in", "out")), (lib.dvbs2_iqconv_pack_device, f, c, ("in", "out"))):
            code_side, float_side = (0, 1) if entry is lib.dvbs2_iqconv_unpack_device else (1, 0)
            #        in  in_stride n ns out out_stride stats   code   the text names
            rows = [(first, 64, -1, 1, second, 64, s, capi.EINVAL, "n_samples"),
                    (first, 64, 8, -1, second, 64, s, capi.EINVAL, "n_streams"),
                    (first, 64, 65, 1, second, 64, s, capi.ESIZE, "n_samples"),
                    (first, 64, 8, 5, second, 64, s, capi.ESIZE, "n_streams"),
                    (0, 64, 8, 1, second, 64, s, capi.EINVAL, "in is null"),
                    (first, 64, 8, 1, 0, 64, s, capi.EINVAL, "out is null"),
                    (first, 64, 8, 1, second, 64, s + 4, capi.EINVAL, "stats"),
                    (first, 7, 8, 2, second, 64, s, capi.EINVAL, "in_stride"),
                    (first, 64, 8, 2, second, 7, s, capi.EINVAL, "out_stride")]
            shifted = [first, second]
            shifted[float_side] += 4
            rows.append((shifted[0], 64, 8, 1, shifted[1], 64, s, capi.EINVAL, names[float_side] + " must be 8-byte aligned"))
            if fmt == M.S16:
                shifted = [first, second]
                shifted[code_side] += 1
                rows.append((shifted[0], 64, 8, 1, shifted[1], 64, s, capi.EINVAL, names[code_side] + " must be 2-byte aligned"))
            for *args, code, name in rows:
                rc = entry(conv._h, args[0] or None, args[1], args[2], args[3], args[4] or None, args[5], args[6], stream() or None)
                assert rc == code and name in lib.dvbs2_last_error().decode(), (fmt, args, rc, lib.dvbs2_last_error())
            # accepted: nothing to do, with and without buffers
            for n, ns in ((0, 1), (8, 0), (0, 0)):
                assert entry(conv._h, None, 1, n, ns, None, 1, s, stream() or None) == capi.OK
        # the host-codes entries
        host = np.zeros(512, np.uint8)
        words = np.array([5, 5, 5], np.uint64)
        for n, src, dst, code, name in ((-1, host.ctypes.data, f, capi.EINVAL, "n_samples"), (65, host.ctypes.data, f, capi.ESIZE, "n_samples"),
                                        (8, None, f, capi.EINVAL, "in is null"), (8, host.ctypes.data, None, capi.EINVAL, "out is null"),
                                        (8, host.ctypes.data, f + 4, capi.EINVAL, "out must be 8-byte aligned")):
            assert lib.dvbs2_iqconv_unpack_to_device(conv._h, src, n, dst, words.ctypes.data) == code and name in lib.dvbs2_last_error().decode(), n
        for n, src, dst, code, name in ((-1, f, host.ctypes.data, capi.EINVAL, "n_samples"), (65, f, host.ctypes.data, capi.ESIZE, "n_samples"),
                                        (8, None, host.ctypes.data, capi.EINVAL, "in is null"), (8, f, None, capi.EINVAL, "out is null"),
                                        (8, f + 4, host.ctypes.data, capi.EINVAL, "in must be 8-byte aligned")):
            assert lib.dvbs2_iqconv_pack_from_device(conv._h, src, n, dst, words.ctypes.data) == code and name in lib.dvbs2_last_error().decode(), n
        assert lib.dvbs2_iqconv_unpack_to_device(conv._h, None, 0, None, None) == capi.OK
        assert lib.dvbs2_iqconv_pack_from_device(conv._h, None, 0, None, None) == capi.OK
        torch.cuda.synchronize()
        assert (d_codes.cpu().numpy() == CODE_FILL).all() and (d_floats.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert st.read() == [[0, 0, 0]] * 4 and words.tolist() == [5, 5, 5] and (host == 0).all()
        conv.close()
    for args in ((3, 1.0, 1, 1), (0, np.nan, 1, 1), (0, 1.0, 0, 1), (0, 1.0, 1, 0)):
        h = C.c_void_p()
        assert lib.dvbs2_iqconv_create(C.byref(h), *args, 0) == capi.EINVAL and not h


# ------------------------------------------------------------------ closed loop through a stream of codes, noise-free
LEAD = 2001


@pytest.fixture(scope="module")
def transmitted():
    return L.shaped_six_frames(LEAD, seed=2027)  # the samples tests/test_agc_gpu.py levels: QPSK 1/4 short, six data frames with dummies


@pytest.mark.parametrize("fmt", (M.U8, M.S16))
def test_closed_loop_through_a_stream_of_codes(transmitted, fmt):
    """shaper -> pack (peak at 0.9 of full scale) -> codes -> unpack -> AGC -> symsync -> plsync -> PL front end -> FEC chain: the
    encoder's input bytes come back, and nothing clipped."""
    import torch
    tx = transmitted
    st, ns, seq, plsc, lead = stream(), tx.ns, L.SEQ6, L.PLSC, LEAD
    peak = float(tx.d_y.abs().max().item())
    to_codes = IqConverter(fmt, np.float32(0.9 / peak), max_samples=ns)
    from_codes = IqConverter(fmt, 1.0, max_samples=ns)
    d_codes = torch.zeros(ns * to_codes.bytes, dtype=torch.uint8, device="cuda")
    d_back = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
    stats = Stats(2)
    to_codes.pack_device(tx.d_y.data_ptr(), ns, ns, 1, d_codes.data_ptr(), ns, d_stats=stats.ptr, stream=st)
    from_codes.unpack_device(d_codes.data_ptr(), ns, ns, 1, d_back.data_ptr(), ns, d_stats=stats.ptr + 24, stream=st)
    torch.cuda.synchronize()
    packed, unpacked = stats.read()
    rms = np.sqrt(unpacked[2] / unpacked[0]) / M.UNIT[fmt]
    print(f"closed loop {M.NAMES[fmt]}: peak {peak:.4f}, statistics {packed} / {unpacked}, rms {rms:.4f} of full scale")
    assert packed[:2] == [ns, 0] and unpacked[:2] == [ns, 0] and packed[2] == unpacked[2]
    codes = d_codes.cpu().numpy().view(M.DTYPE[fmt]).astype(np.int64)
    top = max(abs(int(codes.max()) - M.BIAS[fmt]), abs(int(codes.min()) - M.BIAS[fmt])) / float(M.FULL[fmt])
    assert 0.89 <= top <= 0.91
    # the receiver of tests/test_agc_gpu.py::test_closed_loop_through_the_receiver, the AGC levelling to the shaped samples' own level
    reference = float(torch.linalg.vector_norm(tx.d_y[:2 * lead], dim=1).mean().item())
    agc = Agc(rate=0.05, reference=reference, gain=1.0, max_gain=65536.0, max_samples=ns)
    agc.work_device(d_back.data_ptr(), ns, ns, 1, d_back.data_ptr(), ns, 0, ns, st)
    torch.cuda.synchronize()
    rx = L.timing_and_frames(d_back, ns, L.SPS, L.ROLLOFF, 0, tx.n_all, tol=12)
    behind = rx.recs[rx.recs["sof_index"] >= lead]
    assert rx.state == capi.PLSYNC_LOCKED and behind["plsc"].tolist() == seq
    got = L.decode_frames(rx, plsc, L.GOLD, 0.02, first_sof=lead)
    assert len(got.locked) >= 5
    assert np.array_equal(got.msg, tx.sent[got.data_index])  # the encoder's input bytes
    for o in (rx.sync, agc, to_codes, from_codes):
        o.close()
