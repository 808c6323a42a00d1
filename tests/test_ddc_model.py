"""CPU: the models of the digital down-converter against each other and against the pulse shaper's model, the count rule over sequences
of calls, and the host-only entries of the library (dvbs2_ddc_geometry, _produce, _check, the null-handle answers) against the models. No
device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddc_model as DM
import fec_testlib as T
import pulse_model as PM
from dvbs2rx_amd import capi, ddc_check, ddc_geometry, ddc_produce, ddc_tile, pulse_taps

U = DM.U


def _err():
    return capi.lib.dvbs2_last_error().decode()


def _z(rng, n):
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)


SHAPES = [(1, 1), (1, 7), (2, 1), (2, 5), (3, 2), (3, 3), (3, 4), (8, 7), (8, 8), (8, 9), (8, 17), (8, 3), (50, 11), (256, 300)]  # (D, ntaps)


# ------------------------------------------------------------------ model (a) against model (b)
@pytest.mark.parametrize("D,ntaps", SHAPES + [(4, 4096)])
def test_float32_model_against_float64(D, ntaps):
    """(a) against (b) per component within gamma_ntaps sum_t |h[t]| |z[k D - t]|, gamma_n = n u / (1 - n u), u = 2^-24: a recursive sum
    of n rounded products carries at most n roundings on any term (the product's, then at most n - 1 additions: the first addition, onto
    +0.0, is exact) -- Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1. The samples hold zeros of both
    signs but no denormals, so that no product underflows and the relative model of a rounding holds."""
    rng = np.random.default_rng(100 * D + ntaps)
    h = rng.normal(size=ntaps).astype(np.float32)
    n = 3 * D + 2 * ntaps + 40 if ntaps < 1000 else 4200
    z = _z(rng, n)
    z[5 % n], z[11 % n] = 0.0, complex(-0.0, -0.0)
    hist = _z(rng, ntaps - 1)
    gamma = ntaps * U / (1.0 - ntaps * U)
    for position in (0, 1, D - 1, 5 * D + D // 2):
        for hh in (None, hist):
            a, new_hist = DM.decimate32(h, D, z, position, hh)
            b, mag = DM.decimate64(h, D, z, position, hh)
            assert a.size == b.size == DM.produce(position, D, n) and a.size > 0
            err = np.stack([np.abs(a.real.astype(np.float64) - b.real), np.abs(a.imag.astype(np.float64) - b.imag)], axis=1)
            # (b) itself is rounded, in float64: 2^-52 relative per operation
            assert (err <= gamma * mag * (1 + 2.0 ** -20)).all(), (err / np.maximum(gamma * mag, 1e-300)).max()
            want_hist = np.concatenate([np.zeros(ntaps - 1, np.complex64) if hh is None else hh, z])[n:]
            assert np.array_equal(DM.bits(new_hist), DM.bits(want_hist))


def test_float64_model_is_the_plain_convolution():
    """(b) from position 0 and zero history is np.convolve at every D-th sample: the first output uses the first sample"""
    rng = np.random.default_rng(3)
    for D, ntaps in SHAPES:
        h = rng.normal(size=ntaps).astype(np.float32)
        z = _z(rng, 4 * D + ntaps + 9)
        b, _ = DM.decimate64(h, D, z)
        full = np.convolve(z.astype(np.complex128), h.astype(np.float64))[:z.size:D]
        assert b.size == full.size and np.abs(b - full).max() <= 1e-12 * ntaps


# ------------------------------------------------------------------ cuts
@pytest.mark.parametrize("D,ntaps", SHAPES)
def test_one_call_equals_any_cutting_into_calls(D, ntaps):
    """bit for bit, with cuts of 0 samples, cuts of fewer than D samples, cuts shorter than the history and positions that are no
    multiples of D; ntaps < D, ntaps = 1 and D = 1 are among the shapes"""
    rng = np.random.default_rng(7 * D + ntaps)
    h = rng.normal(size=ntaps).astype(np.float32)
    n = 6 * D + 3 * ntaps + 31
    z = PM.planted(rng, n)
    for start in (0, 3, 7 * D + 1):
        whole, whole_hist = DM.decimate32(h, D, z, start)
        for trial in range(3):
            cuts = [0, 1, max(D - 1, 0), 0, D, D + 1, 2] + [int(c) for c in rng.integers(0, 2 * D + ntaps, 4)]
            rng.shuffle(cuts)
            cuts = [c for c in cuts if c <= n]
            parts, hist, pos = [], None, 0
            for c in cuts + [n]:
                c = min(c, n - pos)
                y, hist = DM.decimate32(h, D, z[pos:pos + c], start + pos, hist)
                assert y.size == DM.produce(start + pos, D, c)
                parts.append(y)
                pos += c
            assert pos == n
            assert np.array_equal(DM.bits(np.concatenate(parts)), DM.bits(whole)), (start, cuts)
            assert np.array_equal(DM.bits(hist), DM.bits(whole_hist))
            assert 0 in cuts and any(c < D for c in cuts)


def test_count_rule_over_sequences_of_calls():
    rng = np.random.default_rng(9)
    for D in (1, 2, 3, 8, 50, 255, 256):
        for start in (0, 1, D - 1, D, 12345, DM.MAX_POSITION - (1 << 25)):
            pos, total = start, 0
            for n_in in [0, 1, D - 1, D, D + 1, DM.MAX_SAMPLES] + [int(c) for c in rng.integers(0, 5000, 8)]:
                n = DM.produce(pos, D, n_in)
                ks = [k for k in range(-(-pos // D), -(-pos // D) + n + 2) if pos <= k * D < pos + n_in] if n_in < 10000 else None
                assert ks is None or len(ks) == n  # the enumeration
                assert n == ddc_produce(pos, D, n_in) and (n_in + D - 1) // D - 1 <= n <= (n_in + D - 1) // D
                pos, total = pos + n_in, total + n
            assert total == DM.produce(start, D, pos - start)  # pieces sum to one call
    assert DM.produce(0, 4, 1) == 1 and DM.produce(1, 4, 3) == 0 and DM.produce(1, 4, 4) == 1  # the first output uses the first sample
    for args in ((-1, 4, 5), (DM.MAX_POSITION + 1, 4, 5), (0, 0, 5), (0, 257, 5), (0, 4, -1), (0, 4, DM.MAX_SAMPLES + 1)):
        assert capi.lib.dvbs2_ddc_produce(*args) == capi.EINVAL and _err() == "position must be in 0..2^62, decim in 1..256, n_in in 0..2^24"
        with pytest.raises(capi.Dvbs2Error):
            ddc_produce(*args)


# ------------------------------------------------------------------ against the pulse shaper's model
@pytest.mark.parametrize("sps,rolloff,delay", [(4, 0.35, 5), (8, 0.2, 5), (2, 0.2, 8)])
def test_matched_filter_peaks_at_the_symbol_instants(sps, rolloff, delay):
    """pulse_model.shape32 shapes symbols with the RRC taps; decimate32 with D = sps and the same taps (scaled to sum 1) is the matched
    filter sampled once per symbol. The combined pulse g = tx * rx is a truncated raised cosine with its centre at 2 sps delay: an
    impulse comes back largest at output 2 delay of the phase that holds the centre and nowhere else as large, and random symbols come
    back as g[centre] x[k - 2 delay] within the intersymbol interference sum_{m != 0} |g[centre + m sps]| max|x| of the truncation plus
    the rounding of both stages (gamma_L sum|tx||x| through sum|rx|, and gamma_ntaps sum|rx||y|, bounded together by
    2 (ntaps + 2) u sum|rx| sum|tx| max|x|)."""
    tx = pulse_taps(sps, rolloff, delay)
    rx = (tx.astype(np.float64) / sps).astype(np.float32)
    ntaps = tx.size
    g = np.convolve(tx.astype(np.float64), rx.astype(np.float64))
    centre = 2 * sps * delay
    assert np.argmax(np.abs(g)) == centre
    impulse = np.zeros(6 * delay + 4, np.complex64)
    impulse[0] = 1.0
    shaped, _ = PM.shape32(tx, sps, impulse)
    peaks = []
    for p in range(sps):  # the sampling phases: drop p samples, so that outputs sit on the samples p + k sps
        y, _ = DM.decimate32(rx, sps, shaped[p:])
        peaks.append((np.abs(y).max(), int(np.argmax(np.abs(y)))))
    assert max(range(sps), key=lambda p: peaks[p][0]) == 0 and peaks[0][1] == 2 * delay
    assert all(peaks[0][0] > peaks[p][0] for p in range(1, sps))
    rng = np.random.default_rng(sps)
    x = ((rng.integers(0, 2, 300) * 2 - 1 + 1j * (rng.integers(0, 2, 300) * 2 - 1)) / np.sqrt(2)).astype(np.complex64)
    shaped, _ = PM.shape32(tx, sps, x)
    y, _ = DM.decimate32(rx, sps, shaped)
    isi = np.sum(np.abs(g[centre % sps::sps])) - abs(g[centre])
    rounding = 2 * (ntaps + 2) * U * np.sum(np.abs(rx.astype(np.float64))) * np.sum(np.abs(tx.astype(np.float64)))
    err = np.abs(y[2 * delay:].astype(np.complex128) - g[centre] * x[:x.size - 2 * delay].astype(np.complex128))
    assert err.max() <= (isi + rounding) * (1 + 1e-6) and isi < abs(g[centre])  # (|x| = 1)
    assert err.max() > 0.05 * isi  # the bound is of the size of the error


# ------------------------------------------------------------------ the host-only entries
def test_geometry_and_tile():
    for D in (1, 2, 3, 8, 50, 256):
        for ntaps in (1, 2, 129, 801, 4096):
            assert ddc_geometry(D, ntaps) == DM.geometry(D, ntaps) == (ntaps - 1, ntaps - 1)
            t = ddc_tile(D, ntaps)
            assert t == DM.tile(D, ntaps) and 20 <= t <= capi.DDC_MAX_TILE and t * D + ntaps - 1 <= capi.DDC_SPAN
    assert ddc_tile(8, 129) == 1024 and ddc_tile(50, 801) == 168 and ddc_tile(256, 4096) == 20
    v = [C.c_int(-7) for _ in range(2)]
    for D, ntaps in ((0, 5), (257, 5), (-1, 5), (4, 0), (4, 4097), (4, -3)):
        assert capi.lib.dvbs2_ddc_geometry(D, ntaps, *[C.byref(x) for x in v]) == capi.EINVAL
        assert _err() == "decim must be in 1..256, ntaps in 1..4096"
    assert [x.value for x in v] == [-7] * 2
    assert capi.lib.dvbs2_ddc_geometry(8, 129, None, None) == capi.OK  # every output is nullable


def test_check_and_create_refuse_bad_arguments_before_any_device():
    """The argument checks come first, so they answer on a machine without a device too."""
    lib, h = capi.lib, C.c_void_p()
    good = np.ones(21, np.float32)
    bad = good.copy()
    bad[7] = np.nan
    big = np.ones(4097, np.float32)
    rows = (((0, good.ctypes.data, 21, 1, 1, 16), "decim must be in 1..256"), ((257, good.ctypes.data, 21, 1, 1, 16), "decim must be in 1..256"),
            ((4, good.ctypes.data, 0, 1, 1, 16), "ntaps must be in 1..4096"), ((4, big.ctypes.data, 4097, 1, 1, 16), "ntaps must be in 1..4096"),
            ((4, None, 21, 1, 1, 16), "null taps"), ((4, bad.ctypes.data, 21, 1, 1, 16), "taps[7] is not finite"),
            ((4, good.ctypes.data, 21, 0, 1, 16), "max_channels out of range (1..65535)"),
            ((4, good.ctypes.data, 21, 65536, 1, 16), "max_channels out of range (1..65535)"),
            ((4, good.ctypes.data, 21, 1, 0, 16), "max_inputs out of range (1..65535)"),
            ((4, good.ctypes.data, 21, 1, 65536, 16), "max_inputs out of range (1..65535)"),
            ((4, good.ctypes.data, 21, 1, 1, 0), "max_samples out of range (1..2^24)"),
            ((4, good.ctypes.data, 21, 1, 1, (1 << 24) + 1), "max_samples out of range (1..2^24)"))
    for args, text in rows:
        assert lib.dvbs2_ddc_check(*args) == capi.EINVAL and _err() == text, args
        assert lib.dvbs2_ddc_create(C.byref(h), *args, 0) == capi.EINVAL and _err() == text, args
        assert not h
    assert lib.dvbs2_ddc_check(1, good.ctypes.data, 1, 1, 1, 1) == capi.OK
    assert lib.dvbs2_ddc_check(256, big.ctypes.data, 4096, 65535, 65535, 1 << 24) == capi.OK
    ddc_check(8, good)
    with pytest.raises(capi.Dvbs2Error):
        ddc_check(300, good)


def test_tile_constants_are_the_header_s():
    hdr = open(os.path.join(T.ROOT, "include", "dvbs2_fec_hip.h")).read()
    assert int(re.search(r"#define DVBS2_DDC_SPAN (\d+)", hdr).group(1)) == capi.DDC_SPAN == DM.SPAN
    assert int(re.search(r"#define DVBS2_DDC_MAX_TILE (\d+)", hdr).group(1)) == capi.DDC_MAX_TILE == DM.MAX_TILE
