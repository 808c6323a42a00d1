"""CPU: the position rule of the resampler against a brute-force enumeration, its two models against each other and against the
continuous design, and the host-only entries of the library (dvbs2_resamp_step, _geometry, _max_out, _check, the null-handle answers)
against the models. No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fec_testlib as T
import pulse_model as PM
import resamp_model as RM
from dvbs2rx_amd import capi, pulse_taps, resamp_check, resamp_geometry, resamp_max_out, resamp_step

U = 2.0 ** -24  # unit roundoff of float32


def _err():
    return capi.lib.dvbs2_last_error().decode()


def _steps(rng):
    """both ends, 1, steps around 1, the rates of the GPU tests, and odd steps that use all 32 fraction bits"""
    fixed = [RM.MIN_STEP, RM.MAX_STEP, 1 << 32, (1 << 32) + 1, (1 << 32) - 1, RM.step_of(2.5), RM.step_of(0.8), RM.step_of(1 + 1e-4),
             RM.MAX_STEP - 1, RM.MIN_STEP + 1]
    return fixed + [int(s) | 1 for s in rng.integers(RM.MIN_STEP, RM.MAX_STEP, 12)]


# ------------------------------------------------------------------ the position rule
def test_produce_equals_the_enumeration_and_pieces_sum_to_one_call():
    rng = np.random.default_rng(41)
    for step in _steps(rng):
        # few enough inputs that the enumeration stays short at the fast end (64 outputs per input)
        most = 40 if step < (1 << 29) else 400
        for acc0 in (0, 1, (1 << 32) - 1, int(rng.integers(0, 1 << 32)), step - 1):
            cuts = [int(c) for c in rng.integers(0, most, 6)] + [0, 1, 0]
            rng.shuffle(cuts)
            acc, pieces, pos = acc0, [], 0
            for n_in in cuts:
                n, after = RM.advance(acc, step, n_in)
                Ts = RM.enumerate_positions(acc, step, n_in)
                assert n == len(Ts) and n <= RM.max_out(step, n_in), (step, acc, n_in)
                assert after == (Ts[-1] + step if Ts else acc) - (n_in << 32) and after >= 0
                assert after < step or n == 0  # a call that produced anything leaves acc below step
                pieces += [t + (pos << 32) for t in Ts]
                pos, acc = pos + n_in, after
            whole = RM.enumerate_positions(acc0, step, pos)
            assert pieces == whole and RM.advance(acc0, step, pos) == (len(whole), acc)


def test_max_out_is_never_exceeded_and_is_reached():
    rng = np.random.default_rng(42)
    for step in _steps(rng):
        for n_in in (0, 1, 2, 37, 1000, RM.MAX_SAMPLES):
            cap = resamp_max_out(step, n_in)
            assert cap == RM.max_out(step, n_in) and cap < 1 << 31
            accs = [0, 1, step - 1, step // 2] + [int(a) for a in rng.integers(0, step, 20)]
            outs = [RM.advance(a, step, n_in)[0] for a in accs]
            assert max(outs) == cap == outs[0] and min(outs) >= cap - 1  # reached at acc = 0; any acc below step loses one at most
    for step, n_in in ((RM.MIN_STEP - 1, 5), (RM.MAX_STEP + 1, 5), (0, 5), (1 << 32, -1), (1 << 32, RM.MAX_SAMPLES + 1)):
        assert capi.lib.dvbs2_resamp_max_out(step, n_in) == capi.EINVAL and _err() == "step must lie in [2^26, 2^33], n_in in 0..2^24"


def test_step():
    for rate in (0.5, 64.0, 1.0, 2.5, 0.8, 1 + 1e-4, 1 - 1e-4, 1 + 2e-5, 63.999, 0.50001, 3.0):
        step = resamp_step(rate)
        assert step == RM.step_of(rate) and RM.MIN_STEP <= step <= RM.MAX_STEP
        assert abs(2.0 ** 32 / step - rate) <= rate * rate * 2.0 ** -33 * (1 + 1e-6)  # half a unit of step
    assert (resamp_step(0.5), resamp_step(1.0), resamp_step(64.0)) == (1 << 33, 1 << 32, 1 << 26)
    out = C.c_uint64(7)
    for rate in (0.4999, 64.001, 0.0, -1.0, float("nan"), float("inf")):
        assert capi.lib.dvbs2_resamp_step(rate, C.byref(out)) == capi.EINVAL and _err() == "rate must lie in [0.5, 64]"
    assert out.value == 7
    assert capi.lib.dvbs2_resamp_step(1.0, None) == capi.EINVAL and _err() == "null step"


def test_split_of_a_position():
    """branch and weight are the top bits of the fraction: (j + a) / nfilts is the fraction itself, to 2^-24 / nfilts"""
    rng = np.random.default_rng(43)
    T_ = [int(t) for t in rng.integers(0, 1 << 40, 200)] + [0, (1 << 32) - 1, 1 << 32, (5 << 32) | 0x07ffffff, (5 << 32) | 0x08000000]
    for lg in range(1, 9):
        i, j, a = RM.split(T_, lg)
        f = np.array([t & 0xffffffff for t in T_], np.float64) / 2.0 ** 32
        assert np.array_equal(i, np.array([t >> 32 for t in T_])) and (j >= 0).all() and (j < 1 << lg).all()
        assert (a >= 0).all() and (a < 1).all()
        back = (j + a.astype(np.float64)) / (1 << lg)
        assert (back <= f).all() and (f - back < 2.0 ** -24 / (1 << lg)).all()


# ------------------------------------------------------------------ model (a) against model (b)
@pytest.mark.parametrize("nfilts,ntaps", [(32, 321), (2, 1), (2, 256), (2, 7), (256, 8192), (256, 1000), (16, 401)])
def test_float32_model_against_float64(nfilts, ntaps):
    """(a) against (b) per component within gamma_{L+2} (sum|h_k||x| + a sum|d_k||x|), gamma_T = T u / (1 - T u), u = 2^-24: each sum is
    a recursive sum of at most L rounded products (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1), and the
    product a * o1 and the last addition bring one rounding each. The samples hold zeros of both signs but no denormals, so that no
    product underflows and the relative model of a rounding holds."""
    rng = np.random.default_rng(1000 * nfilts + ntaps)
    h = rng.normal(size=ntaps).astype(np.float32)
    L, H, _ = RM.geometry(nfilts, ntaps)
    x = (rng.normal(size=300) + 1j * rng.normal(size=300)).astype(np.complex64)
    x[5], x[11], x[200:203] = 0.0, complex(-0.0, -0.0), 0.0
    hist = (rng.normal(size=H) + 1j * rng.normal(size=H)).astype(np.complex64)
    gamma = (L + 2) * U / (1.0 - (L + 2) * U)
    for step, acc in ((RM.step_of(2.5), 0), (RM.step_of(0.8) | 1, 0x9abcdef1), (RM.step_of(1 + 1e-4), (1 << 32) - 5)):
        for hh in (None, hist):
            a, new_hist, acc_after = RM.resample32(h, nfilts, x, step, acc, hh)
            b, mag, _ = RM.resample64(h, nfilts, x, step, acc, hh)
            assert a.size == b.size == RM.advance(acc, step, x.size)[0] and acc_after == RM.advance(acc, step, x.size)[1]
            err = np.stack([np.abs(a.real.astype(np.float64) - b.real), np.abs(a.imag.astype(np.float64) - b.imag)], axis=1)
            # (b) itself is rounded, in float64: 2^-52 relative per operation
            assert (err <= gamma * mag * (1 + 2.0 ** -20)).all(), (err / np.maximum(gamma * mag, 1e-300)).max()
            want_hist = np.concatenate([np.zeros(H, np.complex64) if hh is None else hh, x])[x.size:]
            assert np.array_equal(RM.bits(new_hist), RM.bits(want_hist))


def test_rate_one_at_phase_zero_is_a_plain_fir():
    """step 2^32, acc 0: every output has branch 0 and a = 0, so y = o0 + 0 * o1, which is o0 bit for bit unless o0 is -0.0 (it is
    not: the accumulator starts at +0.0) -- the pulse shaper's model at sps 1 with branch 0's taps."""
    rng = np.random.default_rng(44)
    nfilts = 32
    h = pulse_taps(nfilts, 0.35, 5, 0.0, nfilts)
    x = PM.planted(rng, 500)
    y, hist, acc = RM.resample32(h, nfilts, x, 1 << 32)
    fir, fir_hist = PM.shape32(h[::nfilts].copy(), 1, x)
    assert acc == 0 and y.size == x.size
    assert np.array_equal(RM.bits(y), RM.bits(fir)) and np.array_equal(RM.bits(hist), RM.bits(fir_hist))


def test_model_is_cut_invariant():
    rng = np.random.default_rng(45)
    h = pulse_taps(32, 0.2, 5, 0.0, 32)
    x = PM.planted(rng, 300)
    for step in (RM.step_of(2.5), RM.step_of(0.8), RM.step_of(1 + 1e-4) | 1):
        whole, _, end = RM.resample32(h, 32, x, step, 12345)
        hist, acc, parts, pos = None, 12345, [], 0
        for n in (1, 0, 9, 2, 100, 188):
            y, hist, acc = RM.resample32(h, 32, x[pos:pos + n], step, acc, hist)
            parts.append(y)
            pos += n
        assert pos == x.size and acc == end and np.array_equal(RM.bits(np.concatenate(parts)), RM.bits(whole))


# ------------------------------------------------------------------ model (b) against the continuous design
@pytest.mark.parametrize("nfilts,sps_design,rolloff,D", [(32, 32, 0.2, 5), (32, 32, 0.35, 8), (16, 40, 0.2, 5)])
def test_float64_model_against_the_continuous_design(nfilts, sps_design, rolloff, D):
    """The prototype samples a continuous pulse G at sps_design taps per symbol: h[n] = G((n - c) / sps_design). An output at branch j and
    weight a uses h[n] + a (h[n + 1] - h[n]) for n = j + k nfilts: the chord of G between two neighbouring taps at a / sps_design behind
    the first. A chord over an interval of width w is within max|G''| w^2 / 8 of the function (the error of linear interpolation), here
    w = 1 / sps_design; with the prototype at nfilts taps per input sample that is max|h''| / (8 nfilts^2) per tap in units of the
    prototype's own argument. The comparison filter has the design at the exact position, dvbs2_pulse_taps with tau = -a / sps_design,
    for every tap that has a right neighbour; the prototype's last tap has none (d[ntaps - 1] = 0) and is held, there as here. Rounding
    adds at most 4 u (sum|e_k||x| + sum|h_k||x| + a sum|d_k||x|): taps h, d and e rounded once each to float32, a within 2^-24.
    max|G''| comes from second differences of the float64 design at 16 points per tap, the largest of them raised by the (w / 16)^2
    max|G''''| / 12 that a second difference can fall short, taken from the fourth differences of the same sampling."""
    rng = np.random.default_rng(46)
    h = pulse_taps(sps_design, rolloff, D, 0.0, float(sps_design))
    ntaps = h.size
    fine = 16
    grid = np.stack([PM.taps64(sps_design, np.float64(np.float32(rolloff)), D, -q / (fine * sps_design), float(sps_design)) for q in range(fine)],
                    axis=1).reshape(-1)  # G at spacing w / 16
    w = 1.0 / sps_design
    d2 = np.diff(grid, 2) / (w / fine) ** 2
    d4 = np.diff(grid, 4) / (w / fine) ** 4
    g2 = np.abs(d2).max() + (w / fine) ** 2 * np.abs(d4).max() / 12
    lin = g2 * w * w / 8
    x = (rng.normal(size=120) + 1j * rng.normal(size=120)).astype(np.complex64)
    L, H, _ = RM.geometry(nfilts, ntaps)
    xe = np.concatenate([np.zeros(H, np.complex128), x.astype(np.complex128)])
    worst = 0.0
    for step, acc in ((RM.step_of(2.5), 77), (RM.step_of(1 + 1e-4), 0x7fffff00), (RM.step_of(0.8) | 1, 3)):
        b, mag, (i, j, a) = RM.resample64(h, nfilts, x, step, acc)
        for m in range(b.size):
            e = pulse_taps(sps_design, rolloff, D, -float(a[m]) / sps_design, float(sps_design)).astype(np.float64)
            e[ntaps - 1] = h[ntaps - 1]
            ek = e[j[m]::nfilts]
            xs = xe[H + i[m] - np.arange(ek.size)]
            want = np.sum(ek * xs)
            for c, (got, ref, comp) in enumerate(((b[m].real, want.real, np.abs(xs.real)), (b[m].imag, want.imag, np.abs(xs.imag)))):
                bound = lin * comp.sum() + 4 * U * (np.sum(np.abs(ek) * comp) + mag[m, c])
                assert abs(got - ref) <= bound, (step, m, abs(got - ref), bound)
                worst = max(worst, abs(got - ref) / bound)
    assert worst > 0.01  # the bound is of the size of the error, not orders above it


# ------------------------------------------------------------------ the host-only entries
def test_geometry():
    for nfilts in (2, 4, 8, 16, 32, 64, 128, 256):
        for ntaps in (1, nfilts - 1, nfilts, nfilts + 1, min(nfilts * 128, 8192), 321):
            if ntaps < 1 or -(-ntaps // nfilts) > 128:
                continue
            assert resamp_geometry(nfilts, ntaps) == RM.geometry(nfilts, ntaps)
    v = [C.c_int(-7) for _ in range(3)]
    for nfilts, ntaps in ((0, 5), (1, 5), (3, 5), (48, 5), (512, 5), (-2, 5), (2, 0), (2, 257), (256, 8193), (32, 4097)):
        assert capi.lib.dvbs2_resamp_geometry(nfilts, ntaps, *[C.byref(x) for x in v]) == capi.EINVAL
        assert _err() == "nfilts must be a power of two in 2..256, ntaps in 1..8192 with ceil(ntaps / nfilts) <= 128"
    assert [x.value for x in v] == [-7] * 3
    assert capi.lib.dvbs2_resamp_geometry(32, 321, None, None, None) == capi.OK  # every output is nullable


def test_check_and_create_refuse_bad_arguments_before_any_device():
    """The argument checks come first, so they answer on a machine without a device too."""
    lib, h = capi.lib, C.c_void_p()
    good = np.ones(21, np.float32)
    bad = good.copy()
    bad[7] = np.inf
    big = np.ones(8193, np.float32)
    taps_text = "ntaps must be in 1..8192 with at most 128 taps per branch (ceil(ntaps / nfilts) <= 128)"
    rows = (((3, good.ctypes.data, 21, 1.0, 1, 16), "nfilts must be a power of two in 2..256"),
            ((512, good.ctypes.data, 21, 1.0, 1, 16), "nfilts must be a power of two in 2..256"),
            ((1, good.ctypes.data, 21, 1.0, 1, 16), "nfilts must be a power of two in 2..256"),
            ((2, good.ctypes.data, 0, 1.0, 1, 16), taps_text), ((2, big.ctypes.data, 257, 1.0, 1, 16), taps_text),
            ((256, big.ctypes.data, 8193, 1.0, 1, 16), taps_text), ((2, None, 21, 1.0, 1, 16), "null taps"),
            ((2, bad.ctypes.data, 21, 1.0, 1, 16), "taps[7] is not finite"),
            ((2, good.ctypes.data, 21, 0.49, 1, 16), "rate must lie in [0.5, 64]"), ((2, good.ctypes.data, 21, 64.5, 1, 16), "rate must lie in [0.5, 64]"),
            ((2, good.ctypes.data, 21, float("nan"), 1, 16), "rate must lie in [0.5, 64]"),
            ((2, good.ctypes.data, 21, 1.0, 0, 16), "max_streams out of range (1..65535: streams are one launch dimension)"),
            ((2, good.ctypes.data, 21, 1.0, 65536, 16), "max_streams out of range (1..65535: streams are one launch dimension)"),
            ((2, good.ctypes.data, 21, 1.0, 1, 0), "max_samples out of range (1..2^24)"),
            ((2, good.ctypes.data, 21, 1.0, 1, (1 << 24) + 1), "max_samples out of range (1..2^24)"))
    for args, text in rows:
        assert lib.dvbs2_resamp_check(*args) == capi.EINVAL and _err() == text, args
        assert lib.dvbs2_resamp_create(C.byref(h), *args, 0) == capi.EINVAL and _err() == text, args
        assert not h
    assert lib.dvbs2_resamp_check(2, good.ctypes.data, 21, 1.0, 1, 16) == capi.OK
    assert lib.dvbs2_resamp_check(256, big.ctypes.data, 8192, 64.0, 65535, 1 << 24) == capi.OK
    resamp_check(32, good, 2.5)
    with pytest.raises(capi.Dvbs2Error):
        resamp_check(32, good, 0.25)


def test_tile_constant_is_the_header_s():
    hdr = open(os.path.join(T.ROOT, "include", "dvbs2_fec_hip.h")).read()
    assert int(re.search(r"#define DVBS2_RESAMP_TILE (\d+)", hdr).group(1)) == capi.RESAMP_TILE
