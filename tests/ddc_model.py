"""Models of the digital down-converter (dvbs2_ddc_*): a mixer with the rotator's arithmetic, then a decimating FIR with real taps.

Count rule, Python integers: the handle's sample counter stands at `position`; a call of n_in samples writes the outputs k (absolute) with
position <= k D < position + n_in, that is ceil((position + n_in) / D) - ceil(position / D) of them.

(a) decimate32: step 2 of the definition in float32, operation by operation, on MIXED samples z: y[k] = sum_t h[t] z[k D - t], real and
    imaginary part apart, each term a float32 product and then a float32 addition, t ascending, onto an accumulator that starts at +0.0,
    with the ntaps - 1 samples of history before the call. numpy rounds every array operation to float32 and fuses nothing. The device is
    compared bit for bit with this applied to what the rotator gives on the device for the same input.
(b) decimate64: the same sums in float64 with the magnitude sums of the error bound.
(c) ddc64: mixing from the exact 64-bit phase (plcoarse_model.Rotator) and filtering in float64, with the bound on the mixing error
    carried through the filter."""
import numpy as np

import plcoarse_model as PC

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32
MAX_DECIM, MAX_TAPS, MAX_SAMPLES, MAX_POSITION = 256, 4096, 1 << 24, 1 << 62
SPAN, MAX_TILE = 9216, 1024


def geometry(D, ntaps):
    """(history, delay_num): the delay is delay_num / 2 input samples"""
    return ntaps - 1, ntaps - 1


def produce(position, D, n_in):
    return -(-(position + n_in) // D) - -(-position // D)


def tile(D, ntaps):
    return min(MAX_TILE, (SPAN - (ntaps - 1)) // D)


def _prepare(taps, D, z, position, hist, dtype):
    taps = np.ascontiguousarray(taps, F32)
    z = np.ascontiguousarray(z, np.complex64)
    H = taps.size - 1
    hist = np.zeros(H, np.complex64) if hist is None else np.ascontiguousarray(hist, np.complex64)
    assert hist.size == H and 1 <= D <= MAX_DECIM and position >= 0
    ze = np.concatenate([hist, z])
    n_out = produce(position, D, z.size)
    # output o of the call is absolute output ceil(position / D) + o: it sits on the call's sample (-position) mod D + o D
    newest = H + (-position) % D + D * np.arange(n_out)
    assert n_out == 0 or newest[-1] < ze.size
    return taps, ze, ze.real.astype(dtype), ze.imag.astype(dtype), H, newest


def decimate32(taps, D, z, position=0, hist=None):
    """(a). taps float32, z complex64 mixed samples of one call that starts at the absolute sample `position`, hist the channel's history
    (oldest first) or None for zeros. Returns (produce(position, D, z.size) samples complex64, the history after the call)."""
    taps, ze, re, im, H, newest = _prepare(taps, D, z, position, hist, F32)  # the bits of the input: signed zeros, denormals
    acc_re, acc_im = np.zeros(newest.size, F32), np.zeros(newest.size, F32)
    for t in range(taps.size):
        acc_re = acc_re + taps[t] * re[newest - t]
        acc_im = acc_im + taps[t] * im[newest - t]
        assert acc_re.dtype == F32 and acc_im.dtype == F32
    y = np.stack([acc_re, acc_im], axis=1).reshape(-1).view(np.complex64)
    return y, ze[ze.size - H:].copy()


def decimate64(taps, D, z, position=0, hist=None):
    """(b). Returns (samples complex128, sum_t |h[t]| |z[k D - t]| per component as an (n_out, 2) array)."""
    taps, ze, re, im, H, newest = _prepare(taps, D, z, position, hist, np.float64)
    h = taps.astype(np.float64)
    y = np.zeros(newest.size, np.complex128)
    mag = np.zeros((newest.size, 2))
    for t in range(taps.size):
        y += h[t] * (re[newest - t] + 1j * im[newest - t])
        mag[:, 0] += abs(h[t]) * np.abs(re[newest - t])
        mag[:, 1] += abs(h[t]) * np.abs(im[newest - t])
    return y, mag


def ddc64(taps, D, x, inc):
    """(c). One call from a reset handle: x complex64, inc radians per sample. Returns (samples complex128, the bound on
    |sum_t h[t] (z_device[k D - t] - z_exact[k D - t])| per output), the per-sample mixing bound being plcoarse_model.Rotator's."""
    taps = np.ascontiguousarray(taps, F32).astype(np.float64)
    z, zb = PC.Rotator(inc).work(np.asarray(x, np.complex64))
    H = taps.size - 1
    ze = np.concatenate([np.zeros(H, np.complex128), z])
    be = np.concatenate([np.zeros(H), zb])
    newest = H + D * np.arange(produce(0, D, z.size))
    y = np.zeros(newest.size, np.complex128)
    bound = np.zeros(newest.size)
    for t in range(taps.size):
        y += taps[t] * ze[newest - t]
        bound += abs(taps[t]) * be[newest - t]
    return y, bound


def phase_after(phase, inc_turns, n_in):
    """the 64-bit phase after n_in samples, wrapping"""
    return (phase + n_in * inc_turns) & ((1 << 64) - 1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
