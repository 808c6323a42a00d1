"""CPU: the two models of the pulse shaper against each other, and the host-only entries of the library (dvbs2_pulse_geometry,
dvbs2_pulse_taps, dvbs2_pulse_scale_taps, the null-handle answers) against the models. No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fec_testlib as T
import pulse_model as PM
from dvbs2rx_amd import capi, pulse_geometry, pulse_scale_taps, pulse_taps

U = 2.0 ** -24  # unit roundoff of float32


def _err():
    return capi.lib.dvbs2_last_error().decode()


@pytest.mark.parametrize("sps,ntaps", [(2, 21), (4, 41), (6, 37), (2, 8), (4, 7), (4, 1), (2, 258)])
def test_float32_model_against_float64_convolution(sps, ntaps):
    """(a) against (b) per component within gamma_T sum_k |h_k| |x_{m-k}|, gamma_T = T u / (1 - T u), u = 2^-24, T the number of terms:
    the standard bound for a recursive sum of T rounded products (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
    section 3.1: each product carries one rounding and at most T - 1 additions follow it; the first addition, to +0.0, is exact). The
    symbols hold zeros of both signs but no denormals, so that no product underflows and the relative model of a rounding holds."""
    rng = np.random.default_rng(1000 * sps + ntaps)
    taps = rng.normal(size=ntaps).astype(np.float32)
    x = (rng.normal(size=700) + 1j * rng.normal(size=700)).astype(np.complex64)
    x[5], x[11], x[300:303] = 0.0, complex(-0.0, -0.0), 0.0
    hist = (rng.normal(size=PM.history_of(ntaps, sps)) + 1j * rng.normal(size=PM.history_of(ntaps, sps))).astype(np.complex64)
    for h in (None, hist):
        a, new_hist = PM.shape32(taps, sps, x, h)
        b, mag, terms = PM.shape64(taps, sps, x, h)
        assert a.size == x.size * sps == b.size
        gamma = (terms * U / (1.0 - terms * U))[:, None]
        err = np.stack([np.abs(a.real.astype(np.float64) - b.real), np.abs(a.imag.astype(np.float64) - b.imag)], axis=1)
        # (b) itself is rounded, in float64: 2^-52 relative per operation, 2^-29 of the bound at most
        assert (err <= gamma * mag * (1 + 2.0 ** -20)).all(), (err / np.maximum(gamma * mag, 1e-300)).max()
        assert (err[gamma[:, 0] == 0] == 0).all()  # a phase without taps gives exactly zero
        want_hist = np.concatenate([np.zeros(hist.size, np.complex64) if h is None else h, x])[x.size:]
        assert np.array_equal(PM.bits(new_hist), PM.bits(want_hist))


def test_model_is_cut_invariant():
    rng = np.random.default_rng(3)
    taps = PM.taps64(4, 0.2, 5).astype(np.float32)
    x = PM.planted(rng, 300)
    whole, _ = PM.shape32(taps, 4, x)
    hist, parts, pos = None, [], 0
    for n in (1, 0, 9, 2, 100, 188):
        y, hist = PM.shape32(taps, 4, x[pos:pos + n], hist)
        parts.append(y)
        pos += n
    assert pos == x.size and np.array_equal(PM.bits(np.concatenate(parts)), PM.bits(whole))


def test_geometry():
    for sps in range(2, 65, 2):
        for delay in (1, 64):
            ntaps, history, d = pulse_geometry(sps, delay)
            assert (ntaps, history, d) == (2 * sps * delay + 1, 2 * delay, sps * delay) == PM.geometry(sps, delay)
            assert history == -(-ntaps // sps) - 1 and d == (ntaps - 1) // 2
    v = [C.c_int(-7) for _ in range(3)]
    for sps, delay in ((0, 5), (1, 5), (3, 5), (66, 5), (-2, 5), (2, 0), (2, 65), (2, -1)):
        assert capi.lib.dvbs2_pulse_geometry(sps, delay, *[C.byref(x) for x in v]) == capi.EINVAL
        assert _err() == "sps must be an even integer in 2..64, rrc_delay in 1..64"
    assert [x.value for x in v] == [-7] * 3
    assert capi.lib.dvbs2_pulse_geometry(2, 5, None, None, None) == capi.OK  # every output is nullable


@pytest.mark.parametrize("sps,rolloff,delay", [(2, 0.2, 5), (4, 0.2, 5), (2, 0.35, 20), (6, 0.25, 3), (64, 0.05, 2), (2, 0.0, 4), (8, 1.0, 6),
                                               (4, 0.25, 5)])
def test_designed_taps(sps, rolloff, delay):
    """rolloff 0.25 at sps 4 puts taps on the singular points |t| = 1 / (4 a) = 1."""
    for tau in (0.0, 0.25, -0.25, 0.5, -0.3):
        for gain in (sps, 1.0, -2.5):
            got = pulse_taps(sps, rolloff, delay, tau, gain)
            want = PM.taps64(sps, np.float64(np.float32(rolloff)), delay, tau, gain)
            assert got.dtype == np.float32 and got.size == 2 * sps * delay + 1
            # the criterion of test_symsync_model.py::test_bank: the library's libm against numpy's, then one rounding to float32
            assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max(), (tau, gain)
    h = pulse_taps(sps, rolloff, delay)  # tau = 0, gain = sps
    h64 = h.astype(np.float64)
    assert abs(h64.sum() - sps) <= np.abs(h64).sum() * U  # one rounding per tap
    g = pulse_taps(sps, rolloff, delay, 0.0, 0.75)
    assert abs(g.astype(np.float64).sum() - 0.75) <= np.abs(g.astype(np.float64)).sum() * U
    assert np.array_equal(PM.bits(h), PM.bits(h[::-1]))  # bit-symmetric at tau = 0
    plus, minus = pulse_taps(sps, rolloff, delay, 0.25), pulse_taps(sps, rolloff, delay, -0.25)
    assert np.abs(plus.astype(np.float64) - minus[::-1].astype(np.float64)).max() <= 2.0 ** -23 * np.abs(plus).max()
    assert not np.array_equal(plus, minus)
    # a shift moves the peak: tau > 0 delays the pulse
    assert np.argmax(pulse_taps(sps, rolloff, delay, 0.5)) > np.argmax(pulse_taps(sps, rolloff, delay, -0.5))


def test_designed_taps_refusals():
    buf = np.full(21, -7.0, np.float32)
    lib = capi.lib
    geo = "sps must be an even integer in 2..64, rrc_delay in 1..64"
    rest = "rolloff must lie in [0, 1], tau in [-0.5, 0.5], gain must be finite and not zero"
    for args, text in (((3, 0.2, 5, 0.0, 1.0), geo), ((2, 0.2, 0, 0.0, 1.0), geo), ((66, 0.2, 5, 0.0, 1.0), geo), ((2, -0.1, 5, 0.0, 1.0), rest),
                       ((2, 1.5, 5, 0.0, 1.0), rest), ((2, float("nan"), 5, 0.0, 1.0), rest), ((2, 0.2, 5, 0.51, 1.0), rest),
                       ((2, 0.2, 5, -0.75, 1.0), rest), ((2, 0.2, 5, float("nan"), 1.0), rest), ((2, 0.2, 5, 0.0, 0.0), rest),
                       ((2, 0.2, 5, 0.0, float("inf")), rest), ((2, 0.2, 5, 0.0, float("nan")), rest)):
        assert lib.dvbs2_pulse_taps(*args, buf.ctypes.data) == capi.EINVAL and _err() == text, args
    assert (buf == -7.0).all()
    assert lib.dvbs2_pulse_taps(2, 0.2, 5, 0.0, 2.0, None) == capi.EINVAL and _err() == "null taps"


def test_scale_taps():
    rng = np.random.default_rng(8)
    cases = [(2, pulse_taps(2, 0.2, 5)), (4, pulse_taps(4, 0.35, 5, 0.3)), (6, rng.normal(size=37).astype(np.float32)),
             (4, rng.normal(size=7).astype(np.float32)), (4, np.array([-3.0], np.float32)), (1, rng.normal(size=5).astype(np.float32))]
    for sps, taps in cases:
        for fullscale in (1.0, 0.5, 32767.0):
            got = pulse_scale_taps(taps, sps, fullscale)
            want = PM.scale_taps64(taps, sps, fullscale)
            assert got.dtype == np.float32 and got.shape == taps.shape
            # within one float32 rounding of the rule evaluated in float64
            assert (np.abs(got.astype(np.float64) - want) <= np.abs(want) * U * (1 + 2.0 ** -20)).all(), (sps, fullscale)
            # what the rule promises: no phase's absolute sum exceeds sqrt(2) fullscale, and one reaches it
            peak = max(np.abs(got[p::sps].astype(np.float64)).sum() for p in range(sps))
            assert abs(peak - np.sqrt(2.0) * fullscale) <= np.sqrt(2.0) * fullscale * 2 * U  # one rounding per tap, and the rule's own in float64
    lib, t, zeros, inf = capi.lib, np.ones(4, np.float32), np.zeros(4, np.float32), np.array([1, np.inf, 1, 1], np.float32)
    text = "taps must be ntaps >= 1 finite values that are not all zero, sps >= 1, fullscale finite"
    for args in ((None, 4, 2, 1.0), (t.ctypes.data, 0, 2, 1.0), (t.ctypes.data, 4, 0, 1.0), (t.ctypes.data, 4, 2, float("nan")),
                 (zeros.ctypes.data, 4, 2, 1.0), (inf.ctypes.data, 4, 2, 1.0)):
        assert lib.dvbs2_pulse_scale_taps(*args) == capi.EINVAL and _err() == text, args
    assert (t == 1.0).all() and (zeros == 0.0).all() and inf.tolist() == [1, np.inf, 1, 1]  # a refused call changes nothing


def test_create_refuses_bad_arguments_before_any_device():
    """The argument checks come first, so they answer on a machine without a device too."""
    lib, h = capi.lib, C.c_void_p()
    good = np.ones(21, np.float32)
    bad = good.copy()
    bad[7] = np.inf
    nan = good.copy()
    nan[20] = np.nan
    geo = "sps must be an even integer in 2..64, rrc_delay in 1..64"
    for args, text in (((3, 0.2, 5, 1, 16), geo), ((2, 0.2, 65, 1, 16), geo), ((2, 1.5, 5, 1, 16), "rolloff must lie in [0, 1]"),
                       ((2, 0.2, 5, 0, 16), "max_streams out of range (1..65535: streams are one launch dimension)"),
                       ((2, 0.2, 5, 65536, 16), "max_streams out of range (1..65535: streams are one launch dimension)"),
                       ((2, 0.2, 5, 1, 0), "max_symbols out of range (1..2^30)"), ((2, 0.2, 5, 1, (1 << 30) + 1), "max_symbols out of range (1..2^30)")):
        assert lib.dvbs2_pulse_create(C.byref(h), *args, 0) == capi.EINVAL and _err() == text, args
        assert not h
    terms = "ntaps must be at least 1 and at most 129 taps per phase (ceil(ntaps / sps) <= 129)"
    big = np.ones(259, np.float32)
    for args, text in (((1, good.ctypes.data, 21, 1, 16), "sps must be an even integer in 2..64"),
                       ((66, good.ctypes.data, 21, 1, 16), "sps must be an even integer in 2..64"),
                       ((2, good.ctypes.data, 0, 1, 16), terms), ((2, big.ctypes.data, 259, 1, 16), terms), ((2, None, 21, 1, 16), "null taps"),
                       ((2, bad.ctypes.data, 21, 1, 16), "taps[7] is not finite"), ((2, nan.ctypes.data, 21, 1, 16), "taps[20] is not finite"),
                       ((2, good.ctypes.data, 21, 0, 16), "max_streams out of range (1..65535: streams are one launch dimension)"),
                       ((2, good.ctypes.data, 21, 1, -1), "max_symbols out of range (1..2^30)")):
        assert lib.dvbs2_pulse_create_taps(C.byref(h), *args, 0) == capi.EINVAL and _err() == text, args
        assert not h


def test_tile_constant_is_the_header_s():
    hdr = open(os.path.join(T.ROOT, "include", "dvbs2_fec_hip.h")).read()
    assert int(re.search(r"#define DVBS2_PULSE_TILE (\d+)", hdr).group(1)) == capi.PULSE_TILE
