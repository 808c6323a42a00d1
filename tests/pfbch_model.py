"""Models of the polyphase filter bank channelizer (include/dvbs2_fec_hip.h, dvbs2_pfbch_*): M equally spaced channels of a capture, each
filtered by real taps and decimated by D, with the FIR work done once (M branch sums per output instant) and one M-point transform.

Count rule, Python integers: the down-converter's (ddc_model.produce).

(a) channelize32: the definition in numpy float32, operation by operation. Branch sums w[k][r] = sum over the taps t with
    (k D - t) mod M == r of h[t] x[k D - t], t ascending, real and imaginary part apart, each term a float32 product and then a float32
    addition onto +0.0; then spectrum_model.fft32 over twiddles64(M) rounded once. numpy rounds every array operation to float32 and
    fuses nothing. The device equals this bit for bit.
(b) channelize64: the direct double sum Y[k][c] = sum_t h[t] x[k D - t] e^{-2 pi j c ((k D - t) mod M) / M} with what the error bound
    of (a) against it needs.
(c) bound: |Y32 - Y64| <= sqrt(2) gamma_q S (1 + B) + B ||w||_2 per output (notes/pfbch.md derives it)."""
import math

import numpy as np

import ddc_model as DM
import spectrum_model as SM

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32
MAX_CHAN, MAX_TAPS, MAX_SAMPLES, MAX_POSITION = 256, 4096, 1 << 24, 1 << 62
SPAN, MAX_TILE = 5376, 1024
REGISTER_MAX = 16  # the kernel's switch: M <= 16 in a lane's registers, M >= 32 through LDS
BATCH_POINTS = 2048  # M >= 32: M points each of 2048 / M instants are transformed side by side

produce = DM.produce


def geometry(M, D, ntaps):
    """(history, delay_num, taps per branch): the delay is delay_num / 2 input samples"""
    return ntaps - 1, ntaps - 1, -(-ntaps // M)


def tile(M, D, ntaps):
    return min(MAX_TILE, (SPAN - (ntaps - 1) - M) // D)


def table32(M):
    """the library's table: twiddles64 rounded once"""
    return SM.twiddles64(M).astype(np.complex64)


def _prepare(taps, M, D, x, position, hist):
    taps = np.ascontiguousarray(taps, F32)
    x = np.ascontiguousarray(x, np.complex64)
    H = taps.size - 1
    hist = np.zeros(H, np.complex64) if hist is None else np.ascontiguousarray(hist, np.complex64)
    assert hist.size == H and 1 <= D <= M <= MAX_CHAN and M & (M - 1) == 0 and M >= 2 and position >= 0
    xe = np.concatenate([hist, x])
    n_out = produce(position, D, x.size)
    first = (-position) % D  # the call's first output sits on its input sample `first`
    newest = H + first + D * np.arange(n_out)  # in xe
    residue = (position + first + D * np.arange(n_out, dtype=object)) % M  # of the ABSOLUTE index: Python integers, any position
    assert n_out == 0 or newest[-1] < xe.size
    return taps, xe, H, newest, residue.astype(np.int64)


def branch_sums32(taps, M, D, x, position=0, hist=None):
    """(w real part, w imaginary part) float32 [n_out, M], the history after the call"""
    taps, xe, H, newest, residue = _prepare(taps, M, D, x, position, hist)
    re, im = xe.real.astype(F32), xe.imag.astype(F32)  # the bits of the input: signed zeros, denormals
    k = np.arange(newest.size)
    wr, wi = np.zeros((newest.size, M), F32), np.zeros((newest.size, M), F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for t in range(taps.size):
            r = (residue - t) % M
            wr[k, r] = wr[k, r] + taps[t] * re[newest - t]
            wi[k, r] = wi[k, r] + taps[t] * im[newest - t]
    assert wr.dtype == F32 and wi.dtype == F32
    return wr, wi, xe[xe.size - H:].copy()


def channelize32(taps, M, D, x, position=0, hist=None, channels=None):
    """(a). taps float32, x complex64 samples of one call that starts at the absolute sample `position`, hist the stream's history
    (oldest first) or None for zeros, channels the selection or None for all M. Returns (complex64 [n_sel, produce(position, D,
    x.size)], the history after the call)."""
    wr, wi, hist = branch_sums32(taps, M, D, x, position, hist)
    yr, yi = SM.fft32(wr, wi, table32(M))
    y = np.stack([yr, yi], axis=-1).reshape(yr.shape[0], 2 * M).view(np.complex64)  # [n_out, M]
    sel = list(range(M)) if channels is None else list(channels)
    return np.ascontiguousarray(y.T[sel]), hist


def channelize64(taps, M, D, x, position=0, hist=None):
    """(b). Returns (Y complex128 [M, n_out], S = sum_t |h[t]| |x[k D - t]| per output, ||w||_2 of the M exact branch sums per output)."""
    taps, xe, H, newest, residue = _prepare(taps, M, D, x, position, hist)
    h, xd = taps.astype(np.float64), xe.astype(np.complex128)
    k = np.arange(newest.size)
    w = np.zeros((newest.size, M), np.complex128)
    S = np.zeros(newest.size)
    for t in range(taps.size):
        r = (residue - t) % M
        w[k, r] += h[t] * xd[newest - t]
        S += abs(h[t]) * np.abs(xd[newest - t])
    E = np.exp(-2j * np.pi * np.outer(np.arange(M), np.arange(M)) / M)  # [c, r]
    return E @ w.T, S, np.sqrt((np.abs(w) ** 2).sum(axis=1))


def bound(M, ntaps, S, w_norm):
    """(c), per output and for every channel of it. q = ceil(ntaps / M) terms per branch sum; B = t eta / (1 - t eta), t = log2 M, eta of
    Higham's Theorem 24.2 for the library's table (spectrum_model.fft_eta).
    CAVEAT for whoever sees a test fail against it: this is the bound the stage was specified with, and its transform term is NOT a worst
    case. Theorem 24.2 bounds the 2-norm of the transform's error by B ||F w||_2 = B sqrt(M) ||w||_2; B ||w||_2 per output is that error
    spread evenly over the M outputs. The guaranteed bound is gamma_q S + B sqrt(M) (||w||_2 + gamma_q S) (rigorous_bound below).
    Measured ratios against this one are 0.03 - 0.18, so a ratio above 1 means a defect or an input that piles the transform's error on one
    output, not rounding as usual; compare with rigorous_bound before anything else."""
    q, t = -(-ntaps // M), M.bit_length() - 1
    eta, _ = SM.fft_eta(table32(M), M)
    B = t * eta / (1.0 - t * eta)
    return math.sqrt(2.0) * SM.gamma(q) * S * (1.0 + B) + B * w_norm


def rigorous_bound(M, ntaps, S, w_norm):
    """What the theorem guarantees (see bound): larger than bound() by up to sqrt(M) on the transform term. Not asserted anywhere."""
    q, t = -(-ntaps // M), M.bit_length() - 1
    eta, _ = SM.fft_eta(table32(M), M)
    B = t * eta / (1.0 - t * eta)
    return SM.gamma(q) * S + B * math.sqrt(M) * (w_norm + SM.gamma(q) * S)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
