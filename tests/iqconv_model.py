"""numpy float32 restatement of the IQ sample converter (gr-dvbs2rx_amd/csrc/iqconv_math.hpp): both directions and the statistics.
Every float step is one float32 operation in the order the header writes; the statistics are Python integers."""
import numpy as np

U8, S8, S16 = 0, 1, 2
FORMATS = (U8, S8, S16)
NAMES = {U8: "u8", S8: "s8", S16: "s16"}
DTYPE = {U8: np.uint8, S8: np.int8, S16: np.int16}
BIAS = {U8: np.float32(127.5), S8: np.float32(0), S16: np.float32(0)}
FULL = {U8: np.float32(128), S8: np.float32(128), S16: np.float32(32768)}
LO = {U8: 0, S8: -128, S16: -32768}
HI = {U8: 255, S8: 127, S16: 32767}
MID = {U8: 128, S8: 0, S16: 0}
UNIT = {U8: 256, S8: 128, S16: 32768}  # rms = sqrt(energy / samples) / UNIT
GAIN_MIN, GAIN_MAX = np.float32(2.0 ** -64), np.float32(2.0 ** 64)
M64 = (1 << 64) - 1


def all_codes(fmt):
    return np.arange(LO[fmt], HI[fmt] + 1).astype(DTYPE[fmt])


def level(fmt, codes):
    """d per component as int64: 2 c - 255 for u8, c for the signed formats"""
    c = np.asarray(codes).astype(np.int64)
    return 2 * c - 255 if fmt == U8 else c


def stats_of(fmt, codes, clipped):
    """{samples, clipped, energy} of a row of codes (I, Q, I, Q, ...) as Python ints; clipped: a boolean per component"""
    d = level(fmt, codes).reshape(-1)
    return [d.size // 2, int(np.count_nonzero(clipped)), _energy(d)]


def _energy(d):
    # d * d is below 2^31 and int64 holds 2^32 of them: sum blocks of 2^20 exactly, then in Python
    sq = d * d
    return sum(int(sq[i:i + (1 << 20)].sum()) for i in range(0, sq.size, 1 << 20)) & M64


def unpack(fmt, gain, codes):
    """codes (any shape, the format's dtype) -> float32 of the same shape, and the boolean `on a rail` per component"""
    c = np.asarray(codes)
    assert c.dtype == DTYPE[fmt]
    scale = np.float32(gain) * (np.float32(1) / FULL[fmt])  # exact: a power of two
    v = c.astype(np.float32)
    if fmt == U8:
        v = v - BIAS[fmt]
    y = v * scale
    return y.astype(np.float32), (c == LO[fmt]) | (c == HI[fmt])


def pack(fmt, gain, x):
    """float32 (any shape) -> codes of the same shape, and the boolean `clipped` per component"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = x * np.float32(gain)
        w = t * FULL[fmt]
        if fmt == U8:
            w = w + BIAS[fmt]
        r = np.rint(w)  # to nearest, ties to even
    nan = np.isnan(r)
    below, above = r < LO[fmt], r > HI[fmt]
    safe = np.where(nan | below | above, np.float32(0), r)
    code = np.where(nan, MID[fmt], np.where(below, LO[fmt], np.where(above, HI[fmt], safe.astype(np.int64))))
    return code.astype(DTYPE[fmt]), nan | below | above


def unpack_rows(fmt, gain, codes):
    """codes [ns, n, 2] -> (float32 [ns, n, 2], [[samples, clipped, energy] per row])"""
    y, rail = unpack(fmt, gain, codes)
    return y, [stats_of(fmt, codes[r], rail[r]) for r in range(codes.shape[0])]


def pack_rows(fmt, gain, x):
    """float32 [ns, n, 2] -> (codes [ns, n, 2], [[samples, clipped, energy] per row])"""
    c, clip = pack(fmt, gain, x)
    return c, [stats_of(fmt, c[r], clip[r]) for r in range(c.shape[0])]


def edge_values(fmt):
    """The float32 inputs of pack at gain 1 where it can go wrong: every tie k + 1/2 near both rails and near zero, the first values
    below lo - 1/2 and above hi + 1/2, infinities, NaN, -0, denormals and the largest finite values. Returned as float32; the value x
    stands for the code-domain value x * F + B."""
    full, bias = float(FULL[fmt]), float(BIAS[fmt])
    ks = list(range(LO[fmt] - 3, LO[fmt] + 4)) + list(range(-4, 4)) + list(range(HI[fmt] - 3, HI[fmt] + 4))
    if fmt == U8:
        ks += list(range(124, 132))
    vals = []
    for k in ks:
        for code_value in (k + 0.5, k, k + 0.25, k + 0.75):
            vals.append((code_value - bias) / full)  # exact in float32: at most 19 significant bits
    xs = np.array(vals, np.float32)
    assert np.array_equal(xs.astype(np.float64), np.array(vals, np.float64))
    lo_edge, hi_edge = np.float32((LO[fmt] - 0.5 - bias) / full), np.float32((HI[fmt] + 0.5 - bias) / full)
    around = [np.nextafter(lo_edge, np.float32(-np.inf)), lo_edge, np.nextafter(lo_edge, np.float32(np.inf)),
              np.nextafter(hi_edge, np.float32(-np.inf)), hi_edge, np.nextafter(hi_edge, np.float32(np.inf))]
    fmax = np.finfo(np.float32).max
    special = [np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1e-41, -1e-41, 1.1754944e-38, fmax, -fmax, 1.0, -1.0]
    out = np.concatenate([xs, np.array(around, np.float32), np.array(special, np.float32)])
    if out.size % 2:
        out = np.append(out, np.float32(0.125))
    return out
