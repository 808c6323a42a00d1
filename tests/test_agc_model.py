"""CPU: the float32 model of the AGC (tests/agc_model.py) against itself -- cuts, swap_iq, the cap -- against the fixed point of the
recurrence and against a float64 evaluation under the bound derived in notes/agc.md; and the library's host-only dvbs2_agc_check."""
import numpy as np
import pytest

import agc_model as AM
from dvbs2rx_amd import agc_check, capi

RATE = 1e-2
AMPLITUDES = (0.01, 1.0, 50.0)
N_SETTLE = 120000  # (1 - 1e-2 * 0.01)^120000 = e^-12 of the start distance is left at the weakest amplitude


def planted(rng, ns, n):
    """random complex64 [ns, n] with zeros of both signs and denormals planted"""
    d = rng.normal(size=(ns, n, 2)).astype(np.float32)
    for j, v in enumerate(np.array([0.0, -0.0, 1e-41, -1e-41], np.float32)):
        d[:, (3 + 7 * j) % n, j & 1] = v
    return d.reshape(ns, 2 * n).view(np.complex64)


def test_pieces_equal_one_call():
    rng = np.random.default_rng(1)
    x = planted(rng, 3, 500)
    one = AM.AgcModel(0.05, 1.0, 0.5, 65536.0, 3)
    out, gains = one.work(x)
    cut = AM.AgcModel(0.05, 1.0, 0.5, 65536.0, 3)
    outs, gs, pos = [], [], 0
    lengths = [0, 1, 0] + rng.integers(0, 90, 40).tolist()
    for c in lengths:
        o, g = cut.work(x[:, pos:pos + c])
        assert o.shape == (3, max(0, min(c, 500 - pos))) and g.shape == o.shape
        outs.append(o)
        gs.append(g)
        pos += c
    assert pos >= 500 and lengths.count(0) >= 2  # empty calls among them
    assert np.array_equal(AM.bits(np.concatenate(outs, axis=1)), AM.bits(out))
    assert np.array_equal(AM.bits(np.concatenate(gs, axis=1)), AM.bits(gains))
    assert np.array_equal(AM.bits(cut.g), AM.bits(one.g))
    assert np.array_equal(AM.bits(gains[:, 0]), AM.bits(np.full(3, 0.5, np.float32)))  # the gain BEFORE the update


def test_swap_iq_equals_swapping_the_input():
    x = planted(np.random.default_rng(2), 2, 300)
    a, b = AM.AgcModel(0.05, 1.0, 1.0, 65536.0, 2), AM.AgcModel(0.05, 1.0, 1.0, 65536.0, 2)
    a.swap_iq = True
    swapped = np.ascontiguousarray(x.view(np.float32).reshape(2, 300, 2)[:, :, ::-1]).reshape(2, 600).view(np.complex64)  # the bits, moved
    oa, ga = a.work(x)
    ob, gb = b.work(swapped)
    assert np.array_equal(AM.bits(oa), AM.bits(ob)) and np.array_equal(AM.bits(ga), AM.bits(gb))
    assert not np.array_equal(AM.bits(oa), AM.bits(AM.AgcModel(0.05, 1.0, 1.0, 65536.0, 2).work(x)[0]))


def test_cap_holds_and_zero_never_caps():
    x = AM.constant_envelope(np.random.default_rng(3), 1, 200, 1e-3)
    capped, free = AM.AgcModel(0.5, 1.0, 1.0, 8.0), AM.AgcModel(0.5, 1.0, 1.0, 0.0)
    _, gc = capped.work(x)
    _, gf = free.work(x)
    assert gc.max() == np.float32(8.0) and (gc[0, 20:] == np.float32(8.0)).all() and capped.g[0] == np.float32(8.0)
    assert (np.diff(gf[0]) > 0).all() and gf[0, -1] > 90.0  # no cap: the gain keeps rising towards 1000
    first = int(np.argmax(gc[0] == np.float32(8.0)))
    assert np.array_equal(AM.bits(gc[0, :first]), AM.bits(gf[0, :first]))  # the same until the cap is met


@pytest.fixture(scope="module")
def settled():
    """One run shared by the two tests below: a constant envelope at each amplitude, one stream each."""
    x = AM.constant_envelope(np.random.default_rng(4), len(AMPLITUDES), N_SETTLE, AMPLITUDES)
    m = AM.AgcModel(RATE, 1.0, 1.0, 0.0, len(AMPLITUDES))
    _, gains = m.work(x)
    g32 = np.concatenate([gains, m.g.reshape(-1, 1)], axis=1)
    return x, g32, AM.gains64(x, RATE, 1.0, 1.0, 0.0)


def test_constant_envelope_brings_the_gain_to_ref_over_amplitude(settled):
    x, g32, g64 = settled
    for s, a in enumerate(AMPLITUDES):
        mag = np.hypot(x[s].real.astype(np.float64), x[s].imag.astype(np.float64))
        rate = float(np.float32(RATE))
        left = (1.0 - rate * mag.min()) ** N_SETTLE * abs(1.0 - 1.0 / a)  # what the contraction leaves of the start distance
        spread = max(abs(1.0 / mag.min() - 1.0 / a), abs(1.0 / mag.max() - 1.0 / a))  # the envelope is constant to float32 rounding only
        bound = AM.gain_bound(rate, mag.min(), mag.max(), np.abs(g64[s]).max(), np.abs(1.0 - mag * g64[s, :-1]).max())
        dev = abs(float(g32[s, -1]) - 1.0 / a)
        print(f"amplitude {a}: gain {g32[s, -1]!r}, |gain - ref / A| = {dev:.3e} <= {left + spread + bound:.3e}")
        assert dev <= left + spread + bound


def test_float32_gain_stays_within_the_derived_bound_of_float64(settled):
    """notes/agc.md: |g32 - g64| <= u (3 rate A G + 2 rate D + G) / (rate A). Largest deviation observed / bound, for A = 0.01, 1, 50:
    3.8e-2 / 6.0e-2 (on a gain near 100, whose float32 spacing is 7.6e-6), 4.6e-9 / 6.1e-6, 1.8e-8 / 4.2e-7."""
    x, g32, g64 = settled
    for s, a in enumerate(AMPLITUDES):
        mag = np.hypot(x[s].real.astype(np.float64), x[s].imag.astype(np.float64))
        bound = AM.gain_bound(float(np.float32(RATE)), mag.min(), mag.max(), np.abs(g64[s]).max(), np.abs(1.0 - mag * g64[s, :-1]).max())
        dev = np.abs(g32[s].astype(np.float64) - g64[s]).max()
        print(f"amplitude {a}: largest |g32 - g64| = {dev:.3e}, bound {bound:.3e}")
        assert dev <= bound


def _refused(text, *args):
    assert capi.lib.dvbs2_agc_check(*args) == capi.EINVAL and capi.lib.dvbs2_last_error().decode() == text, capi.lib.dvbs2_last_error()
    with pytest.raises(capi.Dvbs2Error):
        agc_check(*args)


def test_agc_check():
    inf, nan = float("inf"), float("nan")
    for good in ((1e-5, 1.0, 1.0, 65536.0), (0.0, 0.0, 0.0, 0.0), (3e38, -3e38, -1.0, 3e38), (1e-45, 1e-45, 1e-45, 1e-45)):
        assert capi.lib.dvbs2_agc_check(*good) == capi.OK
        agc_check(*good)
    for bad in (-1e-45, -1.0, inf, -inf, nan):
        _refused("rate must be finite and not negative", bad, 1.0, 1.0, 1.0)
        _refused("max_gain must be finite and not negative (0: no cap)", 1e-5, 1.0, 1.0, bad)
    for bad in (inf, -inf, nan):
        _refused("reference must be finite", 1e-5, bad, 1.0, 1.0)
        _refused("gain must be finite", 1e-5, 1.0, bad, 1.0)
    assert capi.AGC_TILE == 64
