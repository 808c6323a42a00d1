"""Models of the pulse shaper (dvbs2_pulse_*): an interpolating FIR by the integer factor sps with real taps over complex symbols.

(a) shape32: the kernel's arithmetic in float32, operation by operation. Output sample m sps + p is the sum over k = 0, 1, ... while
    p + k sps < ntaps of h[p + k sps] x[m - k]: real and imaginary part apart, each term a float32 product and then a float32 addition,
    in ascending k, onto an accumulator that starts at +0.0. numpy rounds every array operation to float32 and fuses nothing. The device
    is compared with this bit for bit.
(b) shape64: np.convolve of the zero-stuffed symbols with the taps in float64.
The designed taps are restated from the closed form (symsync_model.rrc); the scaling rule is the reference's scale_rrc_taps."""
import numpy as np

import symsync_model as S

F32 = np.float32


def geometry(sps, rrc_delay):
    """(ntaps, history in symbols, delay in samples) of the designed taps"""
    ntaps = 2 * sps * rrc_delay + 1
    return ntaps, -(-ntaps // sps) - 1, sps * rrc_delay


def history_of(ntaps, sps):
    return -(-ntaps // sps) - 1


def taps64(sps, rolloff, rrc_delay, tau=0.0, gain=None):
    """the design in float64: the RRC shifted by tau symbols, scaled so that the taps at tau = 0 sum to gain (default sps)"""
    ntaps = 2 * sps * rrc_delay + 1
    g = (np.arange(ntaps) - (ntaps - 1) // 2) / sps
    return S.rrc(g - tau, rolloff) * (sps if gain is None else gain) / np.sum(S.rrc(g, rolloff))


def scale_taps64(taps, sps, fullscale):
    """scale_rrc_taps of the reference's transmit application, in float64"""
    t = np.asarray(taps, np.float64)
    max_sum = max(np.sum(np.abs(t[p::sps])) for p in range(sps))
    return np.sqrt(2.0) * fullscale * t / max_sum


def shape32(taps, sps, x, hist=None):
    """(a). taps float32, x complex64, hist the stream's history (oldest first, complex64) or None for zeros. Returns
    (x.size * sps samples complex64, the history after the call)."""
    taps = np.ascontiguousarray(taps, F32)
    x = np.ascontiguousarray(x, np.complex64)
    H = history_of(taps.size, sps)
    hist = np.zeros(H, np.complex64) if hist is None else np.ascontiguousarray(hist, np.complex64)
    assert hist.size == H
    xe = np.concatenate([hist, x])
    re, im = xe.real.copy(), xe.imag.copy()  # float32, the bits of the input (signed zeros and denormals included)
    n = x.size
    y = np.zeros((n, sps, 2), F32)
    for p in range(sps):
        acc_re, acc_im = np.zeros(n, F32), np.zeros(n, F32)
        for k in range(len(range(p, taps.size, sps))):
            h = taps[p + k * sps]
            acc_re = acc_re + h * re[H - k:H - k + n]
            acc_im = acc_im + h * im[H - k:H - k + n]
            assert acc_re.dtype == F32
        y[:, p, 0], y[:, p, 1] = acc_re, acc_im
    return y.reshape(-1).view(np.complex64), xe[xe.size - H:].copy()


def shape64(taps, sps, x, hist=None):
    """(b). The same in float64 through np.convolve; returns (samples complex128, the bound's sum over k of |h_k| |x_{m-k}| per component
    as an (n sps, 2) array, the number of terms of each sample)."""
    t = np.asarray(taps, np.float64)
    H = history_of(t.size, sps)
    xe = np.concatenate([np.zeros(H, np.complex128) if hist is None else np.asarray(hist, np.complex128), np.asarray(x, np.complex128)])
    up = np.zeros(xe.size * sps, np.complex128)
    up[::sps] = xe
    n = np.asarray(x).size * sps
    y = np.convolve(up, t)[H * sps:H * sps + n]
    mag = np.stack([np.convolve(np.abs(up.real), np.abs(t))[H * sps:H * sps + n], np.convolve(np.abs(up.imag), np.abs(t))[H * sps:H * sps + n]], axis=1)
    terms = np.array([len(range(p, t.size, sps)) for p in range(sps)])
    return y, mag, np.tile(terms, np.asarray(x).size)


def planted(rng, n):
    """n random complex64 symbols with 0.0, -0.0 and denormals of both signs planted in both components"""
    d = rng.normal(size=(n, 2)).astype(F32)
    special = np.array([0.0, -0.0, 1e-41, -1e-41], F32)
    for j, v in enumerate(special):
        d[(3 + 7 * j) % n, 0] = v
        d[(5 + 11 * j) % n, 1] = v
        d[n - 1 - j % n, j & 1] = v
    return d.reshape(-1).view(np.complex64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
