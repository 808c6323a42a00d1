"""Models of the AGC (dvbs2_agc_*): GNU Radio's agc_cc with max_gain behind an optional swap_iq, on a batch of independent streams.

(a) AgcModel: the kernel's arithmetic in float32, operation by operation. Per stream with state g, for every sample (xr, xi) in order
    ((xi, xr) with swap_iq):
        yr = xr * g ; yi = xi * g ; m = sqrt(yr * yr + yi * yi) ; g = g + rate * (ref - m) ; if max_gain > 0 and g > max_gain: g = max_gain
    The model steps through time and holds one float32 per stream in numpy arrays, so every operation is rounded to float32 once and
    nothing is fused; numpy's float32 square root is the correctly rounded one, and denormals are kept. Values that are not finite
    propagate as IEEE says (g > max_gain is false for a NaN). The device is compared with this bit for bit.
(b) gains64: the same recurrence in float64, for the bound of notes/agc.md."""
import numpy as np

F32 = np.float32


class AgcModel:
    def __init__(self, rate=1e-5, reference=1.0, gain=1.0, max_gain=65536.0, n_streams=1):
        self.n_streams = n_streams
        self.gain0 = F32(gain)
        self.swap_iq = False
        self.set_params(rate, reference, max_gain)
        self.reset()

    def set_params(self, rate, reference, max_gain):
        self.rate, self.reference, self.max_gain = F32(rate), F32(reference), F32(max_gain)

    def reset(self):
        self.g = np.full(self.n_streams, self.gain0, F32)

    def set_gain(self, stream_index, gain):
        if stream_index < 0:
            self.g[:] = F32(gain)
        else:
            self.g[stream_index] = F32(gain)

    def work(self, x):
        """x: complex64 [n_streams, n] (or [n] for one stream). Returns (out complex64 [n_streams, n], gains float32 [n_streams, n]:
        the gain that multiplied each sample); the first n_streams' gains move on, as in a call with fewer streams than the handle's."""
        x = np.ascontiguousarray(x, np.complex64)
        x = x.reshape(1, -1) if x.ndim == 1 else x
        ns, n = x.shape
        assert ns <= self.n_streams
        xr, xi = np.ascontiguousarray(x.real.T), np.ascontiguousarray(x.imag.T)  # [n, ns] float32, the bits of the input
        if self.swap_iq:
            xr, xi = xi, xr
        out, gains = np.empty((n, ns, 2), F32), np.empty((n, ns), F32)
        g, rate, ref, cap = self.g[:ns].copy(), self.rate, self.reference, self.max_gain
        with np.errstate(all="ignore"):
            for k in range(n):
                yr, yi = xr[k] * g, xi[k] * g
                m = np.sqrt(yr * yr + yi * yi)
                gains[k] = g
                g = g + rate * (ref - m)
                if cap > 0:
                    g = np.where(g > cap, cap, g)
                assert g.dtype == F32 and m.dtype == F32
                out[k, :, 0], out[k, :, 1] = yr, yi
        self.g[:ns] = g
        return np.ascontiguousarray(out.transpose(1, 0, 2)).reshape(ns, 2 * n).view(np.complex64), np.ascontiguousarray(gains.T)


def gains64(x, rate, reference, gain, max_gain):
    """(b). x complex64 [n_streams, n]; rate, reference, gain, max_gain as the float32 values the model uses, the arithmetic in
    float64 (|x| from the same float32 samples). Returns the gain BEFORE each sample and, last, after the final one: [n_streams, n + 1]."""
    x = np.ascontiguousarray(x, np.complex64)
    mag = np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64)).T
    rate, ref, cap = float(F32(rate)), float(F32(reference)), float(F32(max_gain))
    g = np.full(x.shape[0], float(F32(gain)), np.float64)
    hist = np.empty((mag.shape[0] + 1, x.shape[0]), np.float64)
    for k in range(mag.shape[0]):
        hist[k] = g
        g = g + rate * (ref - mag[k] * g)
        if cap > 0:
            g = np.minimum(g, cap)
    hist[-1] = g
    return np.ascontiguousarray(hist.T)


def gain_bound(rate, a_min, a_max, g_max, d_max):
    """The bound of notes/agc.md on |g32 - g64| at any step for an input whose envelope lies in [a_min, a_max], 0 < rate a_max < 1,
    while |g| <= g_max and |reference - a g| <= d_max: u (3 rate a_max g_max + 2 rate d_max + g_max) / (rate a_min), u = 2^-24, times
    1 + 2^-10 for the terms of second order."""
    u = 2.0 ** -24
    return u * (3 * rate * a_max * g_max + 2 * rate * d_max + g_max) / (rate * a_min) * (1 + 2.0 ** -10)


def constant_envelope(rng, n_streams, n, amplitude):
    """complex64 [n_streams, n]: random phases at the given amplitude (one per stream, or a scalar)"""
    ph = rng.uniform(0, 2 * np.pi, (n_streams, n))
    a = np.broadcast_to(np.asarray(amplitude, np.float64).reshape(-1, 1), (n_streams, 1))
    return (a * np.exp(1j * ph)).astype(np.complex64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
