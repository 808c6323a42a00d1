"""numpy restatement of gr-dvbs2rx_amd/csrc/awgn_math.hpp: Philox4x32-10 words in integer arithmetic, then the float32 Box-Muller with one
array operation per float operation, in the header's order. The host compilation and the device equal it bit for bit. Also the float64
Box-Muller of the same words and the derived bound between the two (notes/awgn.md)."""
import functools

import numpy as np

F = np.float32
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
U64 = (1 << 64) - 1

SQRT2 = np.uint32(0x3FB504F3).view(F)      # 1.41421354
LN2 = np.uint32(0x3F317218).view(F)        # 0.693147182
ANGLE_STEP = np.uint32(0x33490FDB).view(F)  # fl(pi/4) 2^-24
LOG_Q = [F(v) for v in (-0.4999998211860657, 0.3333422541618347, -0.2500249147415161, 0.19953611493110657, -0.1655234396457672,
                        0.1497931331396103, -0.14441822469234467, 0.08733489364385605)]
SIN_S = [F(v) for v in (-0.16666650772094727, 0.00833197869360447, -0.000194956359337084)]
COS_C = [F(v) for v in (-0.5, 0.04166662320494652, -0.0013886763481423259, 2.4390452381339855e-05)]


def philox(counter, key):
    """counter: 4 uint32 (arrays or ints), key: 2 -> the 4 output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k = [int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & MASK]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def words(seed, stream_id, index):
    """(wa, wb) as uint32 arrays for the absolute sample indices `index` (int64 >= 0) of stream `stream_id` (an int, or a uint64 array
    that broadcasts against `index`)."""
    n = np.atleast_1d(np.asarray(index, np.int64))
    assert (n >= 0).all()
    b = (n >> 1).astype(np.uint64)
    seed = int(seed) & U64
    sid = np.asarray(stream_id & U64 if isinstance(stream_id, int) else stream_id, np.uint64)
    w = philox((b & MASK, b >> np.uint64(32), sid & MASK, sid >> np.uint64(32)), (seed & 0xFFFFFFFF, seed >> 32))
    odd = np.broadcast_to((n & 1).astype(bool), w[0].shape)
    return np.where(odd, w[2], w[0]).astype(np.uint32), np.where(odd, w[3], w[1]).astype(np.uint32)


def _horner(coeffs, x):
    acc = np.full(x.shape, coeffs[-1], F)
    for c in coeffs[-2::-1]:
        acc = acc * x + c
    return acc


def radius(wa):
    v = np.uint64(2) * np.asarray(wa, np.uint64) + np.uint64(1)
    e = np.frexp(v.astype(np.float64))[1].astype(np.int64) - 1  # floor(log2 v): v < 2^53 converts exactly
    down, up = np.clip(e - 23, 0, None).astype(np.uint64), np.clip(23 - e, 0, None).astype(np.uint64)
    top = ((v >> down) << up).astype(np.uint32)
    m = (np.uint32(0x3F800000) | (top & np.uint32(0x7FFFFF))).view(F)
    big = m > SQRT2
    m = np.where(big, m * F(0.5), m)
    e = np.where(big, e + 1, e)
    f = m - F(1)
    q = _horner(LOG_Q, f)
    ff = f * f
    l = f + ff * q
    t = (33 - e).astype(F) * LN2 - l
    assert t.dtype == F
    return np.sqrt(F(2) * t)


def angle(wb):
    wb = np.asarray(wb, np.uint32)
    octant = wb >> np.uint32(29)
    p = ((wb >> np.uint32(5)) & np.uint32(0xFFFFFE)) | np.uint32(1)
    p = np.where(octant & np.uint32(1), np.uint32(0x1000000) - p, p)
    a = p.astype(F) * ANGLE_STEP
    z = a * a
    s = _horner(SIN_S, z)
    az = a * z
    sn = a + az * s
    c = _horner(COS_C, z)
    cs = F(1) + z * c
    swap = (((octant + np.uint32(1)) >> np.uint32(1)) & np.uint32(1)).astype(bool)
    x, y = np.where(swap, sn, cs), np.where(swap, cs, sn)
    x = np.where((((octant + np.uint32(2)) >> np.uint32(2)) & np.uint32(1)).astype(bool), -x, x)
    y = np.where((octant >> np.uint32(2)).astype(bool), -y, y)
    assert x.dtype == F and y.dtype == F
    return x, y


def noise_of_words(wa, wb):
    """float32 array [..., 2]: the unit-variance noise (re, im)."""
    r = radius(wa)
    x, y = angle(wb)
    return np.stack([r * x, r * y], axis=-1)


def noise(seed, stream_id, index):
    return noise_of_words(*words(seed, stream_id, index))


def channel(x, sigma, nz):
    """x: float32 [..., 2] or None (noise only); sigma float32 scalar or broadcastable array; one product, then one addition."""
    with np.errstate(all="ignore"):
        scaled = np.asarray(sigma, F) * nz
        return scaled if x is None else np.asarray(x, F) + scaled


def rows(seed, first_stream, first_index, n_samples, n_streams, sigma, x=None):
    """What a call of n_streams rows writes: float32 [n_streams, n_samples, 2]. sigma: scalar or one per row."""
    idx = np.int64(first_index) + np.arange(n_samples, dtype=np.int64)
    sid = np.array([(int(first_stream) + r) & U64 for r in range(n_streams)], np.uint64).reshape(-1, 1)
    nz = noise(seed, sid, idx.reshape(1, -1))
    sig = np.broadcast_to(np.asarray(sigma, F).reshape(-1, 1, 1), (n_streams, 1, 1))
    return channel(x, sig, nz)


# ---- against float64 ----
def reference64(wa, wb):
    """Box-Muller of the same u1 = (wa + 1/2) 2^-32, u2 = (wb + 1/2) 2^-32 in float64: (T = -ln u1, R, re, im)."""
    u1 = (np.asarray(wa, np.float64) + 0.5) * 2.0 ** -32
    u2 = (np.asarray(wb, np.float64) + 0.5) * 2.0 ** -32
    t = -np.log(u1)
    r = np.sqrt(2 * t)
    return t, r, r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)


U = 2.0 ** -24
# notes/awgn.md, "Bound against float64". t: truncation of the mantissa + log1p approximation + log1p evaluation, then the roundings
# that scale with (33 - e) ln 2 <= T + 0.35
DT_ABS = 2.0 ** -23 + 7.0e-9 + 1.36e-7
DT_REL = 2 * U + 2.0 ** -28
# angle: the 6 dropped bits of wb + the rounding of a; then the larger of the two polynomials' approximation + evaluation
D_TRIG = 2 * np.pi * 31.5 * 2.0 ** -32 + (U + 2.9e-8) * 0.7854 + 1.7e-9 + 2.73e-7


def bound64(wa):
    """Per component: |float32 model - float64 reference| <= this, from the float64 T and R of the word."""
    t, r, _, _ = reference64(wa, 0)
    dt = DT_ABS + DT_REL * (t + 0.35)
    dr = np.minimum(np.sqrt(2 * dt), 2 * dt / r)
    dr = dr + U * (r + dr)
    return dr * (1 + D_TRIG) + r * D_TRIG + U * (r + dr) * (1 + D_TRIG)


# ---- the corner words ----
CORNER_SEED, CORNER_STREAM, CORNER_SPAN = 0x5EEDC0DE12345678, 7, 1 << 22


@functools.lru_cache(maxsize=None)
def corner_indices():
    """Among the first 2^22 samples of (CORNER_SEED, CORNER_STREAM): the index with the smallest wa (largest radius), the largest wa,
    and for each of the eight octant boundaries k 2^29 of wb the nearest word below it and the nearest at or above it."""
    wa, wb = words(CORNER_SEED, CORNER_STREAM, np.arange(CORNER_SPAN, dtype=np.int64))
    found = [int(np.argmin(wa)), int(np.argmax(wa))]
    for k in range(8):
        above = wb - np.uint32((k << 29) & 0xFFFFFFFF)  # distance upwards from the boundary, mod 2^32
        found += [int(np.argmax(above)), int(np.argmin(above))]
    return tuple(found)
