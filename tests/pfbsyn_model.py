"""Models of the polyphase synthesis filter bank (include/dvbs2_fec_hip.h, dvbs2_pfbsyn_*): the rows of M equally spaced channels become
one wideband stream at L times their rate, with one M-point inverse transform per input instant and ONE FIR pass for all channels.

Counts, Python integers: a call of n_in instants at the counter k0 writes the n_in L absolute outputs [k0 L, (k0 + n_in) L).

(a) synth32: the definition in numpy float32, operation by operation. Per instant v = (the graph of spectrum_model.fft32 over
    pfbch_model.table32(M) with real and imaginary part exchanged going in and coming out); per output n, with r = n mod M, p = n mod L,
    k1 = n div L: acc = acc + h[p + j L] * v[k1 - j][r] over the existing terms, j DESCENDING, parts apart, from +0.0 or from the tail.
    numpy rounds every array operation to float32 and fuses nothing. The device equals this bit for bit.
(b) synth64: the direct double sum with what the error bound of (a) against it needs.
(c) bound: |y32 - y64| <= gamma_q S + (1 + gamma_q) sum_k |h[n - k L]| B sqrt(M) ||a[k]||_2 per output (notes/pfbsyn.md derives it)."""
import math

import numpy as np

import pfbch_model as PM
import spectrum_model as SM

F32 = np.float32
U = 2.0 ** -24
MAX_CHAN, MAX_TAPS, MAX_SAMPLES, MAX_POSITION, MAX_OUT = 256, 4096, 1 << 24, 1 << 54, 1 << 28
SPAN, SPAN_LONG, MAX_TILE, MAX_PRODUCT = 6144, 13312, 512, 8192
REGISTER_MAX = 16  # the kernel's switch: M <= 16 a lane transforms an instant in registers, M >= 32 two passes through LDS

bits = PM.bits


def geometry(M, L, ntaps):
    """(tail, delay_num, taps per phase): the delay is delay_num / 2 output samples"""
    return max(ntaps - L, 0), ntaps - 1, -(-ntaps // L)


def legal(M, L, ntaps):
    return M in (2, 4, 8, 16, 32, 64, 128, 256) and 1 <= L <= M and 1 <= ntaps <= MAX_TAPS and M * -(-ntaps // L) <= MAX_PRODUCT


def seg_len(M):
    return (M + (M >> 4)) | 1


def tile(M, L, ntaps):
    q = -(-ntaps // L)
    fit = SPAN // seg_len(M) - (q - 1)
    if fit < q:
        fit = SPAN_LONG // seg_len(M) - (q - 1)
    return min(MAX_TILE, fit)


def lds_bytes(M, L, ntaps):
    """what a workgroup asks for: the store of tile + q - 1 instants and the taps"""
    q = -(-ntaps // L)
    return (tile(M, L, ntaps) + q - 1) * seg_len(M) * 8 + ((ntaps + 1) & ~1) * 4


def advance(position, n_in):
    """the counter behind a call, or None where the call is refused"""
    if not (0 <= position <= MAX_POSITION and 0 <= n_in <= MAX_SAMPLES and position + n_in <= MAX_POSITION):
        return None
    return position + n_in


def _rows(M, x, channels):
    """the [n_in, M] inputs of every instant: row i of x in column channels[i], +0.0 elsewhere"""
    x = np.ascontiguousarray(x, np.complex64)
    sel = list(range(M)) if channels is None else list(channels)
    assert x.ndim == 2 and x.shape[0] == len(sel) == len(set(sel)) and all(0 <= c < M for c in sel)
    a = np.zeros((x.shape[1], M), np.complex64)
    a[:, sel] = x.T
    return a


def _terms(M, L, ntaps, position, n_in, j):
    """For the outputs i = 0 .. n_in L + tail - 1 of a call (those at and past n_in L are the tail it leaves) and the term j: which of them
    have it (the tap exists and the instant is one of the call's), the tap, the instant and the residue."""
    tail = max(ntaps - L, 0)
    i = np.arange(n_in * L + tail)
    t = i % L + j * L
    m = i // L - j
    ok = (t <= ntaps - 1) & (m >= 0) & (m < n_in)
    r = ((position * L) % M + i) % M  # position is a Python integer of any size
    return ok, np.minimum(t, ntaps - 1), np.clip(m, 0, max(n_in - 1, 0)), r


def transform32(a, M):
    """(v real part, v imaginary part) float32 [n_in, M]"""
    ar, ai = np.ascontiguousarray(a.real, F32), np.ascontiguousarray(a.imag, F32)  # the bits of the input: signed zeros, denormals
    vi, vr = SM.fft32(ai, ar, PM.table32(M))
    return vr, vi


def synth32(taps, M, L, x, position=0, tail=None, channels=None):
    """(a). taps float32; x complex64 [n_sel, n_in], the rows of one call that starts at the instant `position`; tail the stream's
    partial sums or None for zeros; channels the selection or None for all M. Returns (complex64 [n_in L], the tail after the call)."""
    taps = np.ascontiguousarray(taps, F32)
    ntaps = taps.size
    n_tail, _, q = geometry(M, L, ntaps)
    assert 1 <= L <= M <= MAX_CHAN and M & (M - 1) == 0 and M >= 2 and position >= 0
    a = _rows(M, x, channels)
    n_in = a.shape[0]
    tail = np.zeros(n_tail, np.complex64) if tail is None else np.ascontiguousarray(tail, np.complex64)
    assert tail.size == n_tail
    acc_r, acc_i = np.zeros(n_in * L + n_tail, F32), np.zeros(n_in * L + n_tail, F32)
    acc_r[:n_tail], acc_i[:n_tail] = tail.real, tail.imag
    if n_in:
        vr, vi = transform32(a, M)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for j in range(q - 1, -1, -1):  # the oldest instant first
                ok, t, m, r = _terms(M, L, ntaps, position, n_in, j)
                acc_r[ok] = acc_r[ok] + taps[t[ok]] * vr[m[ok], r[ok]]
                acc_i[ok] = acc_i[ok] + taps[t[ok]] * vi[m[ok], r[ok]]
    assert acc_r.dtype == F32 and acc_i.dtype == F32
    y = np.stack([acc_r, acc_i], axis=-1).reshape(-1).view(np.complex64)
    return y[:n_in * L].copy(), y[n_in * L:].copy()


def synth64(taps, M, L, x, channels=None):
    """(b), from reset. Returns (y complex128 [n_in L], S = sum |h[t]| |v[k][r]| per output, A = sum_k |h[n - k L]| ||a[k]||_2 per
    output). v is the direct sum over the channels, y the direct sum over the instants."""
    taps = np.ascontiguousarray(taps, F32).astype(np.float64)
    ntaps = taps.size
    q = -(-ntaps // L)
    a = _rows(M, x, channels).astype(np.complex128)
    n_in = a.shape[0]
    E = np.exp(2j * np.pi * np.outer(np.arange(M), np.arange(M)) / M)  # [c, r]
    v = a @ E
    a_norm = np.sqrt((np.abs(a) ** 2).sum(axis=1))
    y, S, A = np.zeros(n_in * L, np.complex128), np.zeros(n_in * L), np.zeros(n_in * L)
    for j in range(q):
        ok, t, m, r = (z[:n_in * L] for z in _terms(M, L, ntaps, 0, n_in, j))
        y[ok] += taps[t[ok]] * v[m[ok], r[ok]]
        S[ok] += np.abs(taps[t[ok]]) * np.abs(v[m[ok], r[ok]])
        A[ok] += np.abs(taps[t[ok]]) * a_norm[m[ok]]
    return y, S, A


def bound(M, L, ntaps, S, A):
    """(c), per output. q = ceil(ntaps / L) terms per output; B = t eta / (1 - t eta), t = log2 M, eta of Higham's Theorem 24.2 for the
    library's table (spectrum_model.fft_eta). The theorem is normwise: every element of a transform's error is within
    B ||F a||_2 = B sqrt(M) ||a||_2."""
    q, t = -(-ntaps // L), M.bit_length() - 1
    eta, _ = SM.fft_eta(PM.table32(M), M)
    B = t * eta / (1.0 - t * eta)
    return SM.gamma(q) * S + (1.0 + SM.gamma(q)) * B * math.sqrt(M) * A
