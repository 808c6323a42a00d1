"""CPU: the models of the polyphase synthesizer (tests/pfbsyn_model.py) against each other, against the route the stage replaces, against
the channelizer's model and against the library's host-only entries: the float32 restatement within the derived bound of the double sum,
cuts of a stream bit for bit, the exact route (interpolating FIR per row, mixer, sum), the round trip through the channelizer, special
values, and the geometry, the tile rule and its constants."""
import math
import os
import re

import numpy as np
import pytest

import fec_testlib as T
import pfbch_model as PM
import pfbsyn_model as SY
from dvbs2rx_amd import capi, pfbsyn_check, pfbsyn_geometry, pfbsyn_tile

F32 = np.float32


def rows(seed, n_sel, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n_sel, n)) + 1j * rng.normal(size=(n_sel, n))).astype(np.complex64)


def random_taps(seed, ntaps):
    return (np.random.default_rng(seed).normal(size=ntaps) / math.sqrt(ntaps)).astype(F32)


# ------------------------------------------------------------------ the float32 restatement under the bound
@pytest.mark.parametrize("M,L,ntaps", [(2, 2, 5), (4, 4, 33), (8, 4, 65), (8, 3, 40), (16, 16, 129), (64, 32, 513), (8, 8, 3), (256, 128, 1025)])
def test_float32_model_within_the_bound(M, L, ntaps):
    """|y32 - y64| <= gamma_q S + (1 + gamma_q) sum_k |h[n - k L]| B sqrt(M) ||a[k]||_2 per output (notes/pfbsyn.md). Normal inputs on
    every channel, normal taps / sqrt(ntaps)."""
    taps, x = random_taps(M + ntaps, ntaps), rows(L + ntaps, M, 60 + 2 * -(-ntaps // L))
    y32, _ = SY.synth32(taps, M, L, x)
    y64, S, A = SY.synth64(taps, M, L, x)
    b = SY.bound(M, L, ntaps, S, A)
    err = np.abs(y32.astype(np.complex128) - y64)
    some = b > 0  # (an output without a term, ntaps < L, is +0.0 on both sides and its bound is 0)
    ratio = float((err[some] / b[some]).max())
    print(f"M {M} L {L} ntaps {ntaps}: worst error / bound {ratio:.4f}, worst error {err.max():.3e}, output rms {np.sqrt(np.mean(np.abs(y64) ** 2)):.3f}")
    assert y32.shape == (x.shape[1] * L,) and some.sum() >= min(ntaps, L) * 60 and (err <= b).all() and ratio <= 1.0


# ------------------------------------------------------------------ cuts
@pytest.mark.parametrize("M,L,ntaps", [(8, 3, 40), (16, 8, 5), (8, 4, 4), (8, 4, 1), (4, 1, 9), (8, 5, 23), (256, 128, 4096)])
def test_cuts_give_the_bits_of_one_call(M, L, ntaps):
    """One call equals any cutting, bit for bit: cuts of 0, 1, 2 and 40 instants and the rest, with the selection changed between them
    (what a channel is fed outside its calls is zero, so the one call is fed the rows of every cut at their channels). L not dividing M,
    ntaps < L, ntaps = L, ntaps = 1, L = 1, a tail longer than a call, and the largest bank."""
    taps = random_taps(ntaps, ntaps)
    rng = np.random.default_rng(M * L + ntaps)
    cuts = [3, 0, 1, 2, 40, 0, 7]
    n = sum(cuts)
    whole_in = np.zeros((M, n), np.complex64)
    parts, pos, tail = [], 0, None
    for i, c in enumerate(cuts):
        sel = list(range(M)) if i % 3 == 0 else [int(v) for v in rng.permutation(M)[:max(1, M // 2)]]
        x = rows(1000 * i + M, len(sel), c)
        whole_in[sel, pos:pos + c] = x
        y, tail = SY.synth32(taps, M, L, x, pos, tail, sel)
        assert y.shape == (c * L,) and tail.shape == (max(ntaps - L, 0),)
        parts.append(y)
        pos += c
    whole, tail_whole = SY.synth32(taps, M, L, whole_in)
    assert np.array_equal(SY.bits(np.concatenate(parts)), SY.bits(whole))
    assert np.array_equal(SY.bits(tail), SY.bits(tail_whole))
    # and from a counter that is no multiple of M / L, far out: the residue is that of the absolute output
    far = (1 << 53) + 12345
    a, ta = SY.synth32(taps, M, L, whole_in[:, :9], far)
    b1, tb = SY.synth32(taps, M, L, whole_in[:, :4], far)
    b2, tb = SY.synth32(taps, M, L, whole_in[:, 4:9], far + 4, tb)
    assert np.array_equal(SY.bits(np.concatenate([b1, b2])), SY.bits(a)) and np.array_equal(SY.bits(ta), SY.bits(tb))


# ------------------------------------------------------------------ the exact route
@pytest.mark.parametrize("M,L,ntaps,sel", [(8, 4, 33, [6, 1, 3]), (8, 3, 40, None), (4, 4, 9, [3, 0]), (16, 5, 7, [9, 2, 15, 4])])
def test_double_sum_against_the_route_it_replaces(M, L, ntaps, sel):
    """y[n] = sum_c e^{+2 pi j c n / M} (interpolating FIR by L of row c)[n]: relative 1e-12."""
    taps = random_taps(7, ntaps)
    n_sel = M if sel is None else len(sel)
    x = rows(3, n_sel, 50)
    got, _, _ = SY.synth64(taps, M, L, x, sel)
    n = np.arange(50 * L)
    want = np.zeros(50 * L, np.complex128)
    for i, c in enumerate(range(M) if sel is None else sel):
        up = np.zeros(50 * L, np.complex128)
        up[::L] = x[i]
        want += np.exp(2j * np.pi * c * n / M) * np.convolve(up, taps.astype(np.float64))[:50 * L]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _channelize_direct(g, M, L, y, c):
    """Y[c][k] = sum_t g[t] y[k L - t] e^{-2 pi j c (k L - t) / M} in double, y[n] = 0 for n < 0: the channelizer's meaning, restated"""
    n = np.arange(y.size)
    return np.convolve(y * np.exp(-2j * np.pi * c * n / M), g.astype(np.float64))[:y.size:L]


@pytest.mark.parametrize("M,L,sel,exact", [(4, 3, [3, 0, 1], True), (4, 2, [1, 2], True), (8, 4, [6, 1, 3, 4], False)])
def test_round_trip_through_the_channelizer_model(M, L, sel, exact):
    """pfbch_model.channelize64(g, M, L, .) on synth64's output returns row c as x_c through h * g at the instants k L, relative 1e-10,
    with a scrambled selection on both sides: sign and numbering are the channelizer's. One row is fed at a time: with several, each
    channel also holds what the others leak through h and g, which is no rounding error (the closed loop on the device has it).
    channelize64 takes its input as complex64. At M 4 with small integers for the symbols and eighths for h the wideband stream is
    exact in float32 (the mixers are 1, j, -1, -j), so nothing is lost there; at M 8 the same check runs on the channelizer's meaning
    restated in double, which pfbch_model's tests hold channelize64 against."""
    ntaps = 41
    rng = np.random.default_rng(M + L)
    g = random_taps(2, 29)
    if exact:
        h = (rng.integers(-8, 9, ntaps) / 8.0).astype(F32)
        x = (rng.integers(-4, 5, (len(sel), 80)) + 1j * rng.integers(-4, 5, (len(sel), 80))).astype(np.complex64)
    else:
        h, x = random_taps(1, ntaps), rows(5, len(sel), 80)
    hg = np.convolve(h.astype(np.float64), g.astype(np.float64))
    for i, c in enumerate(sel):
        one = np.zeros_like(x)
        one[i] = x[i]
        y, _, _ = SY.synth64(h, M, L, one, sel)
        if exact:
            assert np.abs(y - y.astype(np.complex64)).max() <= 1e-13
            Y, _, _ = PM.channelize64(g, M, L, y)
            got, mirror = Y[sel][i], Y[(M - c) % M]
        else:
            got, mirror = _channelize_direct(g, M, L, y, c), _channelize_direct(g, M, L, y, (M - c) % M)
        up = np.zeros(80 * L, np.complex128)
        up[::L] = x[i].astype(np.complex128)
        want = np.convolve(up, hg)[:80 * L:L]
        assert got.shape == want.shape == (80,)
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), c
        if (M - c) % M != c:
            assert np.abs(mirror - want).max() > 0.1 * np.abs(want).max()  # the mirror channel does not hold it


# ------------------------------------------------------------------ special values
def test_special_values_are_the_float32_operations_own():
    """An infinite and a NaN sample make exactly the outputs whose taps reach their instants non-finite and leave every other output the
    bits it has without them; denormals are kept; an output starts at +0.0, so -0.0 in gives +0.0 out; an instant that does not exist
    is skipped (0 * inf would be a NaN)."""
    M, L, ntaps = 8, 3, 11
    taps, x = random_taps(3, ntaps), rows(4, M, 120)
    clean, _ = SY.synth32(taps, M, L, x)
    bad = x.copy()
    bad[2, 30] = np.complex64(complex(np.inf, 1.0))
    bad[5, 80] = np.complex64(complex(2.0, np.nan))
    got, _ = SY.synth32(taps, M, L, bad)
    n = np.arange(got.size)
    reached = ((n >= 30 * L) & (n < 30 * L + ntaps)) | ((n >= 80 * L) & (n < 80 * L + ntaps))
    assert reached.sum() == 2 * ntaps
    assert (~np.isfinite(got[reached])).all()
    assert np.array_equal(SY.bits(got[~reached]), SY.bits(clean[~reached]))
    # one tap of 1.0 and L = M = 4: output 4 k is +0.0 + v[k][0] and the other phases have no term; one fed channel at c = 0: v[k][r] = a
    tiny = np.zeros((1, 4), np.complex64)
    tiny[0, 1] = np.complex64(complex(1e-41, -1e-41))
    tiny[0, 2] = np.complex64(complex(-0.0, -0.0))
    y, tail = SY.synth32(np.ones(1, F32), 4, 4, tiny, channels=[0])
    assert y.shape == (16,) and tail.size == 0
    assert y[4].real == F32(1e-41) and y[4].imag == F32(-1e-41) and F32(1e-41) != 0
    assert (SY.bits(y[5:]) == 0).all() and (SY.bits(y[0:4]) == 0).all()  # +0.0, not -0.0; phases 1..3 have no tap
    # an infinite first instant: the outputs before the call have no term at all, and the first outputs not a 0 * inf from instants < 0
    first = np.zeros((1, 3), np.complex64)
    first[0, 0] = np.complex64(complex(np.inf, 0.0))
    y, _ = SY.synth32(random_taps(9, 9), 4, 2, first, channels=[0])
    assert not np.isnan(y.real).any()


# ------------------------------------------------------------------ geometry, tile, constants
def test_geometry_and_tile_are_the_library_s():
    for M, L, ntaps in ((2, 1, 1), (2, 2, 4096), (8, 3, 40), (256, 256, 4096), (256, 128, 4096), (256, 1, 32), (64, 32, 1025), (16, 8, 257),
                        (32, 31, 33), (8, 4, 3), (2, 1, 4096), (256, 24, 257)):
        assert SY.legal(M, L, ntaps)
        assert pfbsyn_geometry(M, L, ntaps) == SY.geometry(M, L, ntaps)
        assert pfbsyn_tile(M, L, ntaps) == SY.tile(M, L, ntaps) >= 1
    for M, L, ntaps in ((256, 1, 33), (256, 127, 4096), (2, 1, 4097), (6, 2, 5), (8, 9, 5), (8, 0, 5)):
        assert not SY.legal(M, L, ntaps)
        with pytest.raises(capi.Dvbs2Error):
            pfbsyn_tile(M, L, ntaps)
    with pytest.raises(capi.Dvbs2Error, match="n_chan \\* ceil\\(ntaps / interp\\) must not exceed 8192"):
        pfbsyn_check(256, 1, np.ones(33, F32))
    pfbsyn_check(256, 1, np.ones(32, F32))


def test_every_legal_shape_launches():
    """The enumeration of notes/pfbsyn.md: every M, every L in 1..M and every q = ceil(ntaps / L) that creation accepts, with the longest
    filter of that q (the tile and the store depend on ntaps through q alone, and the taps add 4 ceil2(ntaps) bytes): the tile is at
    least 1 and the request within 120 KiB, the cap the kernel is allowed."""
    worst_lds, least_tile, shapes = (0, None), (1 << 30, None), 0
    for t in range(1, 9):
        M = 1 << t
        for L in range(1, M + 1):
            for q in range(1, min(SY.MAX_PRODUCT // M, -(-SY.MAX_TAPS // L)) + 1):
                ntaps = min(SY.MAX_TAPS, q * L)
                assert SY.legal(M, L, ntaps) and -(-ntaps // L) == q
                tile, lds = SY.tile(M, L, ntaps), SY.lds_bytes(M, L, ntaps)
                assert tile >= 1 and lds <= SY.SPAN_LONG * 8 + SY.MAX_TAPS * 4 == 120 * 1024, (M, L, ntaps)
                worst_lds = max(worst_lds, (lds, (M, L, ntaps)))
                least_tile = min(least_tile, (tile, (M, L, ntaps)))
                shapes += 1
                if q in (1, 2, 11, 12) or ntaps == SY.MAX_TAPS:
                    assert pfbsyn_tile(M, L, ntaps) == tile
    print(f"{shapes} shapes: largest request {worst_lds}, smallest tile {least_tile}")
    assert least_tile[0] == 12 and least_tile[1][0] == 256


def test_tile_constants_are_the_header_s():
    hdr = open(os.path.join(T.ROOT, "include", "dvbs2_fec_hip.h")).read()
    for name, mine, lib in (("SPAN", SY.SPAN, capi.PFBSYN_SPAN), ("SPAN_LONG", SY.SPAN_LONG, capi.PFBSYN_SPAN_LONG),
                            ("MAX_TILE", SY.MAX_TILE, capi.PFBSYN_MAX_TILE), ("MAX_PRODUCT", SY.MAX_PRODUCT, capi.PFBSYN_MAX_PRODUCT)):
        assert int(re.search(rf"#define DVBS2_PFBSYN_{name} (\d+)", hdr).group(1)) == mine == lib
