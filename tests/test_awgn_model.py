"""CPU: the arithmetic of the AWGN channel stage. The generator against its known answers, the host compilation of awgn_math.hpp
(dvbs2_awgn_words / dvbs2_awgn_sample) against the numpy float32 restatement bit for bit, the restatement against a float64 Box-Muller
under the bound notes/awgn.md derives, the statistics of the model, and dvbs2_awgn_sigma."""
import ctypes as C
import math

import numpy as np
import pytest

import awgn_model as M
from dvbs2rx_amd import blocks as B
from dvbs2rx_amd import capi

KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
SEEDS = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
STAT_SEED, STAT_STREAM = 20261019, 3


def _lib_words(seed, stream_id, index):
    w = np.zeros(2, np.uint32)
    assert capi.lib.dvbs2_awgn_words(seed, stream_id, index, w.ctypes.data) == capi.OK
    return int(w[0]), int(w[1])


def _lib_samples(seed, stream_id, indices):
    out = np.zeros((len(indices), 2), np.float32)
    for j, i in enumerate(indices):
        assert capi.lib.dvbs2_awgn_sample(seed, stream_id, int(i), out.ctypes.data + 8 * j) == capi.OK
    return out


def _corner_words():
    idx = np.array(M.corner_indices(), np.int64)
    return idx, M.words(M.CORNER_SEED, M.CORNER_STREAM, idx)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answers_model_and_library(counter, key, want):
    assert tuple(int(w) for w in M.philox(counter, key)) == want
    # through the entry: counter = (lo32(n >> 1), hi32(n >> 1), lo32(s), hi32(s)), key = (lo32(k), hi32(k)). An index is an int64
    # >= 0, so the entry reaches the counters whose second word is below 2^30: of the second and third answer it takes the other
    # five words as they are and the second counter word cut to 30 bits, and must then equal the model, which the answers pinned
    n2, s, k = counter[0] | (counter[1] & 0x3FFFFFFF) << 32, counter[2] | counter[3] << 32, key[0] | key[1] << 32
    cut = tuple(int(w) for w in M.philox((counter[0], counter[1] & 0x3FFFFFFF, counter[2], counter[3]), key))
    assert (cut == want) == (counter[1] < 1 << 30)
    assert _lib_words(k, s, 2 * n2) + _lib_words(k, s, 2 * n2 + 1) == cut
    assert B.awgn_words(k, s, 2 * n2 + 1) == cut[2:]


def test_word_selection_carry_and_stream_id():
    seed = SEEDS[0]
    for s in (0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        for n in (0, 1, 2, 3, (1 << 33) - 1, 1 << 33, (1 << 33) + 1, (1 << 63) - 1):
            b = n >> 1
            w = [int(x) for x in M.philox((b & 0xFFFFFFFF, b >> 32, s & 0xFFFFFFFF, s >> 32), (seed & 0xFFFFFFFF, seed >> 32))]
            want = (w[2], w[3]) if n & 1 else (w[0], w[1])
            wa, wb = M.words(seed, s, n)
            assert (int(wa[0]), int(wb[0])) == want == _lib_words(seed, s, n), (s, n)
    # the block index crosses 2^32 between 2^33 - 1 and 2^33: the carry goes into the second counter word
    assert _lib_words(seed, 0, (1 << 33) - 1) != _lib_words(seed, 0, (1 << 33) + 1) != _lib_words(seed, 0, 1)
    # the two halves of the stream id are two counter words: 2^32 is not 1 and not 0
    assert len({_lib_words(seed, s, 0) for s in (0, 1, 1 << 32, (1 << 32) - 1, (1 << 64) - 1)}) == 5
    assert capi.lib.dvbs2_awgn_words(0, 0, -1, np.zeros(2, np.uint32).ctypes.data) == capi.EINVAL and b"index" in capi.lib.dvbs2_last_error()
    assert capi.lib.dvbs2_awgn_words(0, 0, 0, None) == capi.EINVAL and b"wa_wb" in capi.lib.dvbs2_last_error()
    assert capi.lib.dvbs2_awgn_sample(0, 0, -1, np.zeros(2, np.float32).ctypes.data) == capi.EINVAL and b"index" in capi.lib.dvbs2_last_error()
    assert capi.lib.dvbs2_awgn_sample(0, 0, 0, None) == capi.EINVAL and b"re_im" in capi.lib.dvbs2_last_error()


def test_model_constants_are_the_headers():
    assert float(M.SQRT2) == 1.41421353816986083984375 and float(M.LN2) == 0.693147182464599609375
    assert M.ANGLE_STEP == np.float32(np.float32(np.pi / 4) * np.float32(2.0 ** -24))


@pytest.mark.parametrize("seed", SEEDS)
def test_host_equals_model_bit_for_bit(seed):
    idx = np.arange(1 << 16, dtype=np.int64) + (5 if seed == SEEDS[1] else 0)
    want = M.noise(seed, 11, idx)
    got = _lib_samples(seed, 11, idx)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(want).all() and (M.radius(M.words(seed, 11, idx)[0]) > 0).all()


def test_host_equals_model_at_the_corner_words():
    idx, (wa, wb) = _corner_words()
    assert wa[0] < 1 << 14 and wa[1] > (1 << 32) - (1 << 14)  # 2^22 draws: an extreme 2^14 from its end has probability e^-16
    assert M.radius(wa[:1])[0] > 4.9 and M.radius(wa[1:2])[0] < 3e-3  # sqrt(-2 ln 2^-18) = 4.995, sqrt(2 * 2^-18) = 2.8e-3
    want = M.noise_of_words(wa, wb)
    got = _lib_samples(M.CORNER_SEED, M.CORNER_STREAM, idx)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(B.awgn_sample(M.CORNER_SEED, M.CORNER_STREAM, idx[0]).view(np.uint32), want[0].view(np.uint32))
    # the words that no search finds: the ends of wa and the octant boundaries of wb themselves
    wa = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    r = M.radius(wa)
    assert np.isfinite(r).all() and (r > 0).all() and abs(float(r[0]) - math.sqrt(2 * 33 * math.log(2))) < 1e-5
    edges = np.array([(k << 29) + d & 0xFFFFFFFF for k in range(8) for d in (-1, 0, 63, 64)], np.uint32)
    x, y = M.angle(edges)
    assert (x != 0).all() and (y != 0).all()
    # the eight-fold symmetry is exact: the words on either side of a boundary mirror each other across it, so they share their two
    # magnitudes -- in place across an axis, exchanged across a diagonal
    pairs = np.sort(np.abs(np.stack([x, y], axis=-1)), axis=-1)
    assert np.array_equal(pairs[0::4], pairs[1::4]) and np.array_equal(pairs[2::4], pairs[1::4]) and not np.array_equal(pairs[3::4], pairs[1::4])


def test_model_against_float64_under_the_derived_bound():
    """notes/awgn.md: with dt = DT_ABS + DT_REL (T + 0.35), dr = min(sqrt(2 dt), 2 dt / R) + u (R + dr), every component is within
    dr (1 + D_TRIG) + R D_TRIG + u (R + dr)(1 + D_TRIG) of the float64 Box-Muller of the same words."""
    cidx, (cwa, cwb) = _corner_words()
    worst = 0.0
    for seed in SEEDS:
        wa, wb = M.words(seed, 11, np.arange(1 << 16, dtype=np.int64))
        wa, wb = np.concatenate([wa, cwa, np.array([0, 0xFFFFFFFF], np.uint32)]), np.concatenate([wb, cwb, np.array([5, 0xFFFFFFFF], np.uint32)])
        got = M.noise_of_words(wa, wb).astype(np.float64)
        _, _, re, im = M.reference64(wa, wb)
        err = np.maximum(np.abs(got[:, 0] - re), np.abs(got[:, 1] - im))
        bound = M.bound64(wa)
        worst = max(worst, float((err / bound).max()))
        print(f"seed {seed:#x}: largest error {err.max():.3e}, largest error / bound {(err / bound).max():.3f}, bound at R = 1: {float(M.bound64(np.uint32(0x9B4597E3))):.3e}")
        assert (err <= bound).all()
    assert worst <= 1.0


def _normal_cdf(x):
    return np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x])


def test_statistics_of_the_model():
    """Seed 20261019, stream 3: 2^20 complex samples = N = 2^21 real values. Thresholds at about five standard deviations of each
    statistic's sampling distribution (Kolmogorov: P(sqrt(N) D > 2.2) = 1.2e-4)."""
    n_cplx = 1 << 20
    idx = np.arange(n_cplx, dtype=np.int64)
    z = M.noise(STAT_SEED, STAT_STREAM, idx).astype(np.float64)
    v = z.reshape(-1)
    N = v.size
    assert N == 1 << 21
    mean, var = v.mean(), v.var()
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1) <= 5 * math.sqrt(2 / N)
    s = np.sort(v)
    cdf = _normal_cdf(s)
    k = np.arange(1, N + 1)
    D = max((k / N - cdf).max(), (cdf - (k - 1) / N).max())
    assert D <= 2.2 / math.sqrt(N)
    corr_bound = 5 / math.sqrt(N / 2)
    other = M.noise(STAT_SEED, STAT_STREAM + 1, idx).astype(np.float64)

    def corr(a, b):
        return float(np.corrcoef(a, b)[0, 1])
    c_ri, c_next, c_stream = corr(z[:, 0], z[:, 1]), corr(v[:-2], v[2:]), corr(v, other.reshape(-1))
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} D {D:.3e} corr re/im {c_ri:.3e} next {c_next:.3e} stream {c_stream:.3e} max {np.abs(v).max():.3f}")
    assert abs(c_ri) <= corr_bound and abs(c_next) <= corr_bound and abs(c_stream) <= corr_bound
    assert np.abs(v).max() <= 6.8


def test_sigma_rule_and_refusals():
    for esn0 in (-3.0, 0.0, 10.0):
        for sps in (1, 2, 4):
            for es in (1.0, 0.37):
                want = math.sqrt(es / 10 ** (esn0 / 10) * sps / 2)
                got = float(B.awgn_sigma(esn0, es, sps))
                # evaluated in double and rounded once: one float32 ulp covers a last-bit difference between two double power functions
                assert abs(got - want) <= want * 2.0 ** -23
    assert float(B.awgn_sigma(0.0, 1.0, 1)) == float(np.float32(math.sqrt(0.5)))
    s = C.c_float(7.0)
    for args, name in [((math.nan, 1.0, 1), b"esn0_db"), ((math.inf, 1.0, 1), b"esn0_db"), ((0.0, math.nan, 1), b"es "), ((0.0, math.inf, 1), b"es "),
                       ((0.0, 0.0, 1), b"es "), ((0.0, -1.0, 1), b"es "), ((0.0, 1.0, 0), b"sps"), ((0.0, 1.0, -2), b"sps"), ((-800.0, 1e300, 1), b"esn0_db and es")]:
        assert capi.lib.dvbs2_awgn_sigma(*args, C.byref(s)) == capi.EINVAL and capi.lib.dvbs2_last_error().startswith(name), args
        assert s.value == 7.0
    assert capi.lib.dvbs2_awgn_sigma(0.0, 1.0, 1, None) == capi.EINVAL
    with pytest.raises(capi.Dvbs2Error):
        B.awgn_check(-1.0)
    B.awgn_check(0.0, 65535, 1 << 30)
