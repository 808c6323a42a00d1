"""CPU: the arithmetic of the IQ sample converter. The numpy float32 restatement (tests/iqconv_model.py) against an independent
evaluation that is exact -- rationals for the codes, float64 products and sums cast once to float32, an integer rounding rule written
out -- and the host compilation of iqconv_math.hpp (dvbs2_iqconv_unpack_host / dvbs2_iqconv_pack_host) against the restatement. Every
check is an equality."""
import os
import re

import numpy as np
import pytest

import fec_testlib as T
import iqconv_model as M
from dvbs2rx_amd import blocks as B
from dvbs2rx_amd import capi

GAINS = (0.3, 16.0, 2.0 ** -64, 2.0 ** 64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exact_pack(fmt, gain, x):
    """pack without the model: float64 products and sums that are exact, each cast once to float32; the rounding to an integer and the
    clamp in Python. Returns (codes, clipped) as lists."""
    full, bias = float(M.FULL[fmt]), float(M.BIAS[fmt])
    codes, clipped = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for v in np.asarray(x, np.float32).reshape(-1):
            t = np.float32(np.float64(v) * np.float64(np.float32(gain)))  # 24 x 24 bits: exact in float64
            u = np.float32(np.float64(t) * full)                           # a power of two: exact, or past FLT_MAX and then infinite
            w = np.float32(np.float64(u) + bias) if bias else u           # decided (|u| >= 2^30) or exact in float64
            if np.isnan(w):
                codes.append(M.MID[fmt]); clipped.append(True)
                continue
            if np.isinf(w):
                codes.append(M.HI[fmt] if w > 0 else M.LO[fmt]); clipped.append(True)
                continue
            lo = int(np.floor(np.float64(w)))
            frac = float(w) - lo  # exact: w is a float32
            r = lo + (1 if frac > 0.5 or (frac == 0.5 and lo % 2) else 0)
            clipped.append(r < M.LO[fmt] or r > M.HI[fmt])
            codes.append(min(max(r, M.LO[fmt]), M.HI[fmt]))
    return codes, clipped


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_unpack_of_every_code_is_the_rational(fmt):
    c = M.all_codes(fmt)
    assert c.size == (65536 if fmt == M.S16 else 256)
    ci = c.astype(np.int64)
    want = (2 * ci - 255) / 256.0 if fmt == M.U8 else ci / float(M.FULL[fmt])  # exact in float64
    y, rail = M.unpack(fmt, 1.0, c)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), want)
    assert np.array_equal(np.nonzero(rail)[0], [0, c.size - 1])
    for g in GAINS:
        g32 = np.float32(g)
        correctly_rounded = (want * np.float64(g32)).astype(np.float32)  # at most 17 x 24 bits: the float64 product is exact
        assert np.array_equal(bits(M.unpack(fmt, g32, c)[0]), bits(correctly_rounded)), g


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_pack_of_unpack_is_the_code(fmt):
    c = M.all_codes(fmt)
    back, clipped = M.pack(fmt, 1.0, M.unpack(fmt, 1.0, c)[0])
    assert np.array_equal(back, c) and not clipped.any()
    for e in (-64, -7, 1, 12, 64):
        g = np.float32(2.0 ** e)
        back, clipped = M.pack(fmt, np.float32(1) / g, M.unpack(fmt, g, c)[0])
        assert np.array_equal(back, c) and not clipped.any(), e


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_pack_edges_against_the_exact_evaluation(fmt):
    x = M.edge_values(fmt)
    for g in (1.0, 0.3, 16.0, 2.0 ** -64, 2.0 ** 64, 0.5):
        codes, clipped = M.pack(fmt, g, x)
        want_codes, want_clipped = exact_pack(fmt, g, x)
        assert codes.astype(np.int64).tolist() == want_codes and clipped.tolist() == want_clipped, g
    # and spelled out, at gain 1: ties go to the even neighbour, the rails hold, the special values
    full, bias, lo, hi = float(M.FULL[fmt]), float(M.BIAS[fmt]), M.LO[fmt], M.HI[fmt]

    def one(code_value):
        c, k = M.pack(fmt, 1.0, np.array([(code_value - bias) / full], np.float32))
        return int(c[0]), bool(k[0])

    for k in list(range(lo, lo + 3)) + list(range(-3, 3)) + list(range(hi - 3, hi)):
        if lo <= k and k + 1 <= hi:
            assert one(k + 0.5) == (k if k % 2 == 0 else k + 1, False), k
    assert one(lo - 0.5) == (lo, False) and one(hi + 0.5) == (hi, True)  # lo is even: the tie goes onto it; hi is odd: past it
    assert one(lo - 0.25) == (lo, False) and one(hi + 0.25) == (hi, False)  # rounds onto the rail: not clipped
    assert one(lo - 0.75) == (lo, True) and one(hi + 0.75) == (hi, True)
    below = np.nextafter(np.float32((lo - 0.5 - bias) / full), np.float32(-np.inf))
    above = np.nextafter(np.float32((hi + 0.5 - bias) / full), np.float32(np.inf))
    c, k = M.pack(fmt, 1.0, np.array([below, above], np.float32))
    assert c.tolist() == [lo, hi] and k.tolist() == [True, True]
    fmax = np.finfo(np.float32).max
    c, k = M.pack(fmt, 1.0, np.array([np.inf, -np.inf, np.nan, fmax, -fmax, -0.0, 1e-45, -1e-41], np.float32))
    zero = 128 if fmt == M.U8 else 0  # 127.5 is a tie: to the even 128
    assert c.tolist() == [hi, lo, M.MID[fmt], hi, lo, zero, zero, zero]
    assert k.tolist() == [True, True, True, True, True, False, False, False]


def test_ties_at_the_rails():
    """-0.5 is a tie between -1 and 0 and goes to 0: on the rail, not clipped. 255.5 goes to 256: clipped."""
    c, k = M.pack(M.U8, 1.0, np.array([(-0.5 - 127.5) / 128, (255.5 - 127.5) / 128], np.float32))
    assert c.tolist() == [0, 255] and k.tolist() == [False, True]
    c, k = M.pack(M.S16, 1.0, np.array([-32768.5 / 32768, 32767.5 / 32768], np.float32))
    assert c.tolist() == [-32768, 32767] and k.tolist() == [False, True]


def test_statistics():
    # a rail is counted in unpack, and not in pack for a value that rounds onto it
    for fmt in M.FORMATS:
        rails = np.array([[M.LO[fmt], M.HI[fmt]], [M.MID[fmt], M.HI[fmt]]], M.DTYPE[fmt])[None]
        y, st = M.unpack_rows(fmt, 1.0, rails)
        d = [int(v) for v in M.level(fmt, rails).reshape(-1)]
        assert st == [[2, 3, sum(v * v for v in d)]]
        c, st2 = M.pack_rows(fmt, 1.0, y)
        assert np.array_equal(c, rails) and st2 == [[2, 0, st[0][2]]]
        onto = np.array([[(M.HI[fmt] + 0.25 - float(M.BIAS[fmt])) / float(M.FULL[fmt]), 4.0]], np.float32)[None]
        c, st3 = M.pack_rows(fmt, 1.0, onto)
        assert c.reshape(-1).tolist() == [M.HI[fmt]] * 2 and st3[0][:2] == [1, 1]
    assert M.level(M.U8, np.array([0, 127, 128, 255], np.uint8)).tolist() == [-255, -1, 1, 255]
    # the largest energy a row of 2^16 samples can have
    row = np.full((1, 1 << 16, 2), 32767, np.int16)
    assert M.unpack_rows(M.S16, 1.0, row)[1] == [[1 << 16, 1 << 17, (1 << 17) * 32767 * 32767]]
    row[:] = -32768
    assert M.unpack_rows(M.S16, 1.0, row)[1] == [[1 << 16, 1 << 17, (1 << 17) << 30]]


def _lib_unpack(fmt, gain, codes, offset=0):
    """through the C entry, the codes at `offset` bytes into a buffer"""
    raw = np.zeros(codes.nbytes + offset + 8, np.uint8)
    raw[offset:offset + codes.nbytes] = codes.reshape(-1).view(np.uint8)
    out = np.zeros(codes.size, np.float32)
    st = np.zeros(3, np.uint64)
    assert capi.lib.dvbs2_iqconv_unpack_host(fmt, float(np.float32(gain)), raw.ctypes.data + offset, codes.size // 2, out.ctypes.data,
                                             st.ctypes.data) == capi.OK
    return out, [int(v) for v in st]


def _lib_pack(fmt, gain, x, offset=0):
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    width = np.dtype(M.DTYPE[fmt]).itemsize
    raw = np.full(x.size * width + offset + 8, 0xA5, np.uint8)
    st = np.zeros(3, np.uint64)
    assert capi.lib.dvbs2_iqconv_pack_host(fmt, float(np.float32(gain)), x.ctypes.data, x.size // 2, raw.ctypes.data + offset, st.ctypes.data) == capi.OK
    assert (raw[:offset] == 0xA5).all() and (raw[offset + x.size * width:] == 0xA5).all()
    return raw[offset:offset + x.size * width].copy().view(M.DTYPE[fmt]), [int(v) for v in st]


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_library_host_entries_equal_the_model(fmt):
    rng = np.random.default_rng(100 + fmt)
    codes = rng.integers(M.LO[fmt], M.HI[fmt] + 1, (1, 4096, 2)).astype(M.DTYPE[fmt])
    x = np.concatenate([(rng.normal(size=2 * 4096) * 0.6).astype(np.float32), M.edge_values(fmt)]).reshape(1, -1, 2)
    for gain in (1.0, 0.3, 16.0):
        for offset in (0, 2) if fmt == M.S16 else (0, 1):
            y, st = M.unpack_rows(fmt, gain, codes)
            got, got_st = _lib_unpack(fmt, gain, codes, offset)
            assert np.array_equal(bits(got), bits(y).reshape(-1)) and got_st == st[0]
            c, st = M.pack_rows(fmt, gain, x)
            got, got_st = _lib_pack(fmt, gain, x, offset)
            assert np.array_equal(got, c.reshape(-1)) and got_st == st[0]
    every = M.all_codes(fmt).reshape(1, -1, 2)
    assert np.array_equal(bits(_lib_unpack(fmt, 1.0, every)[0]), bits(M.unpack(fmt, 1.0, every)[0]).reshape(-1))
    # the statistics are added to, and the Python helpers are the same entries
    st = np.array([5, 6, 7], np.uint64)
    out = np.zeros(4, np.float32)
    two = np.array([M.LO[fmt], 1, 2, M.HI[fmt]], M.DTYPE[fmt])
    assert capi.lib.dvbs2_iqconv_unpack_host(fmt, 1.0, two.ctypes.data, 2, out.ctypes.data, st.ctypes.data) == capi.OK
    want = M.unpack_rows(fmt, 1.0, two.reshape(1, 2, 2))[1][0]
    assert [int(v) for v in st] == [5 + want[0], 6 + want[1], 7 + want[2]]
    y, d = B.iqconv_unpack_host(M.NAMES[fmt], 0.3, codes[0], stats=True)
    assert np.array_equal(bits(y.view(np.float32)), bits(M.unpack(fmt, 0.3, codes)[0]).reshape(-1))
    assert [d["samples"], d["clipped"], d["energy"]] == M.unpack_rows(fmt, 0.3, codes)[1][0]
    c, d = B.iqconv_pack_host(fmt, 0.3, x.reshape(-1).view(np.complex64), stats=True)
    assert c.dtype == M.DTYPE[fmt] and np.array_equal(c, M.pack(fmt, 0.3, x)[0][0])
    assert [d["samples"], d["clipped"], d["energy"]] == M.pack_rows(fmt, 0.3, x)[1][0]
    assert B.iqconv_bytes(M.NAMES[fmt]) == 2 * np.dtype(M.DTYPE[fmt]).itemsize and B.iqconv_bytes(3) == -1


def test_host_entries_refuse():
    buf = np.zeros(8, np.float32)
    for entry in (capi.lib.dvbs2_iqconv_unpack_host, capi.lib.dvbs2_iqconv_pack_host):
        for args, name in (((3, 1.0, buf.ctypes.data, 1, buf.ctypes.data, None), "format"), ((0, 0.0, buf.ctypes.data, 1, buf.ctypes.data, None), "gain"),
                           ((0, 1.0, buf.ctypes.data, -1, buf.ctypes.data, None), "n is"), ((0, 1.0, None, 1, buf.ctypes.data, None), "in is"),
                           ((0, 1.0, buf.ctypes.data, 1, None, None), "out is")):
            assert entry(*args) == capi.EINVAL and name in capi.lib.dvbs2_last_error().decode(), args
        assert entry(0, 1.0, None, 0, None, None) == capi.OK
    assert (buf == 0).all()
    B.iqconv_check("s16", 2.0 ** 64, 65535, 1 << 30)
    with pytest.raises(capi.Dvbs2Error) as e:
        B.iqconv_check("u8", 2.0 ** 65)
    assert e.value.code == capi.EINVAL and "gain" in str(e.value)


def test_constants_are_the_header_s():
    hdr = open(os.path.join(T.ROOT, "include", "dvbs2_fec_hip.h")).read()

    def defined(name):
        return int(re.search(r"#define %s (\d+)" % name, hdr).group(1))

    assert (defined("DVBS2_IQ_U8"), defined("DVBS2_IQ_S8"), defined("DVBS2_IQ_S16")) == (capi.IQ_U8, capi.IQ_S8, capi.IQ_S16) == M.FORMATS
    assert defined("DVBS2_IQCONV_TILE") == capi.IQCONV_TILE == B.IqConverter.TILE
    assert B.IQ_FORMATS == {v: k for k, v in M.NAMES.items()}
