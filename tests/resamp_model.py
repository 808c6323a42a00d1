"""Models of the arbitrary-rate resampler (dvbs2_resamp_*): a polyphase bank of nfilts branches of a prototype h with linear interpolation
between neighbouring branches through the derivative taps d, real taps over complex samples.

Position rule, Python integers: step counts input samples per output sample with 32 fractional bits; output m of a call of n_in samples
from position acc sits at T = acc + m step and is produced while T < N = n_in << 32; afterwards acc' = acc + n_out step - N. From T:
i = T >> 32 the newest input sample used, f = T & 0xffffffff, branch j = f >> (32 - lg), a = float32((f << lg mod 2^32) >> 8) * 2^-24.

(a) resample32: the kernel's arithmetic in float32, operation by operation: o0 = sum_k h[j + k nfilts] x[i - k], o1 the same with d,
    k ascending while j + k nfilts < ntaps, real and imaginary part apart, each term a float32 product and then a float32 addition onto
    an accumulator that starts at +0.0; y = o0 + a * o1. numpy rounds every array operation to float32 and fuses nothing. The device is
    compared with this bit for bit.
(b) resample64: the same sums in float64 from the same float32 h, d and a, with the magnitude sums of the error bound."""
import numpy as np

F32 = np.float32
MIN_STEP, MAX_STEP, MAX_SAMPLES = 1 << 26, 1 << 33, 1 << 24


def step_of(rate):
    """nearbyint(2^32 / rate) in double (ties to even, as np.rint)"""
    assert 0.5 <= rate <= 64
    return int(np.rint(4294967296.0 / rate))


def geometry(nfilts, ntaps):
    """(terms L, history, delay_num)"""
    L = -(-ntaps // nfilts)
    return L, L - 1, (ntaps - 1) // 2


def advance(acc, step, n_in):
    """(n_out, acc') of one call"""
    N = n_in << 32
    n = 0 if acc >= N else -(-(N - acc) // step)
    return n, acc + n * step - N


def max_out(step, n_in):
    return -(-(n_in << 32) // step)


def enumerate_positions(acc, step, n_in):
    """brute force: every T = acc + m step below N, one by one"""
    N, T, out = n_in << 32, acc, []
    while T < N:
        out.append(T)
        T += step
    return out


def split(T, lg):
    """(i int64, j int64, a float32) of the positions T (Python integers)"""
    T = np.array(T, dtype=np.uint64).reshape(-1)
    f = T & np.uint64(0xffffffff)
    i = (T >> np.uint64(32)).astype(np.int64)
    j = (f >> np.uint64(32 - lg)).astype(np.int64)
    low = ((f << np.uint64(lg)) & np.uint64(0xffffffff)) >> np.uint64(8)  # the 24 bits below the branch bits
    a = low.astype(F32) * F32(2.0 ** -24)
    assert (a.astype(np.float64) * 2.0 ** 24 == low).all()  # the conversion is exact
    return i, j, a


def diff_taps(h):
    """d[n] = h[n + 1] - h[n], d[ntaps - 1] = 0, one float32 subtraction each"""
    h = np.ascontiguousarray(h, F32)
    d = np.zeros(h.size, F32)
    d[:-1] = h[1:] - h[:-1]
    return d


def _sums(h, d, nfilts, re, im, H, i, j, a, dtype):
    """o0 + a o1 per component in `dtype`, and the magnitudes sum|h||x| + a sum|d||x| per component in float64"""
    n = i.size
    y = np.zeros((n, 2), dtype)
    mag = np.zeros((n, 2), np.float64)
    for b in np.unique(j):
        sel = np.nonzero(j == b)[0]
        at = H + i[sel]
        o0 = [np.zeros(sel.size, dtype), np.zeros(sel.size, dtype)]
        o1 = [np.zeros(sel.size, dtype), np.zeros(sel.size, dtype)]
        m0, m1 = np.zeros((sel.size, 2)), np.zeros((sel.size, 2))
        for k in range(len(range(b, h.size, nfilts))):
            hk, dk = dtype(h[b + k * nfilts]), dtype(d[b + k * nfilts])
            for c, x in enumerate((re, im)):
                xv = x[at - k].astype(dtype)
                o0[c] = o0[c] + hk * xv
                o1[c] = o1[c] + dk * xv
                assert o0[c].dtype == dtype and o1[c].dtype == dtype
                m0[:, c] += abs(float(hk)) * np.abs(xv.astype(np.float64))
                m1[:, c] += abs(float(dk)) * np.abs(xv.astype(np.float64))
        aa = a[sel].astype(dtype)
        for c in range(2):
            y[sel, c] = o0[c] + aa * o1[c]
            mag[sel, c] = m0[:, c] + aa.astype(np.float64) * m1[:, c]
    return y, mag


def _prepare(h, nfilts, x, step, acc, hist):
    h = np.ascontiguousarray(h, F32)
    x = np.ascontiguousarray(x, np.complex64)
    lg = nfilts.bit_length() - 1
    assert 1 << lg == nfilts and 2 <= nfilts <= 256
    H = geometry(nfilts, h.size)[1]
    hist = np.zeros(H, np.complex64) if hist is None else np.ascontiguousarray(hist, np.complex64)
    assert hist.size == H
    xe = np.concatenate([hist, x])
    n_out, acc_after = advance(acc, step, x.size)
    i, j, a = split([acc + m * step for m in range(n_out)], lg)
    assert n_out == 0 or (i[-1] < x.size and i[0] >= 0)
    return h, diff_taps(h), xe, H, i, j, a, acc_after


def resample32(h, nfilts, x, step, acc=0, hist=None):
    """(a). h float32, x complex64, hist the stream's history (oldest first) or None for zeros. Returns (n_out samples complex64, the
    history after the call, acc after the call)."""
    h, d, xe, H, i, j, a, acc_after = _prepare(h, nfilts, x, step, acc, hist)
    y, _ = _sums(h, d, nfilts, xe.real.copy(), xe.imag.copy(), H, i, j, a, F32)  # the bits of the input: signed zeros, denormals
    return y.reshape(-1).view(np.complex64), xe[xe.size - H:].copy(), acc_after


def resample64(h, nfilts, x, step, acc=0, hist=None):
    """(b). Returns (samples complex128, the bound's magnitudes (n_out, 2), (i, j, a))."""
    h, d, xe, H, i, j, a, _ = _prepare(h, nfilts, x, step, acc, hist)
    y, mag = _sums(h, d, nfilts, xe.real.copy(), xe.imag.copy(), H, i, j, a, np.float64)
    return y[:, 0] + 1j * y[:, 1], mag, (i, j, a)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
