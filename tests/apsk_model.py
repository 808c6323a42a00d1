"""16APSK / 32APSK soft demapping (DVB-S2 MODCODs 18-28): a float64 model and a float32 restatement of the kernel.

The constellation tables are typed in from EN 302 307-1 5.4.3 / 5.4.4 (ring ratios of tables 9 and 10), independently of the
library's C table. They are UNPINNED: the reference has neither a modulator nor a demapper for these constellations; what is
checked is their internal consistency (unique labels, Es = 1, Gray walks on the rings) and that model and library agree.

Conventions (include/dvbs2_fec_hip.h): entry i of a table is the point with label i; label bit n_mod-1 (the most significant)
is the first interleaver column; LLR < 0 means bit 1; the LLR of column c of symbol j is byte c * rows + j of the frame;
L_b = (min_{bit b = 1} |y - s|^2 - min_{bit b = 0} |y - s|^2) / N0, llr = sat8(rint(L_b)).
"""
import numpy as np

MOD_16APSK, MOD_32APSK = 6, 8
N_MOD = {MOD_16APSK: 4, MOD_32APSK: 5}

GAMMA_16 = {"C2_3": 3.15, "C3_4": 2.85, "C4_5": 2.75, "C5_6": 2.70, "C8_9": 2.60, "C9_10": 2.57}
GAMMA_32 = {"C3_4": (2.84, 5.27), "C4_5": (2.72, 4.87), "C5_6": (2.64, 4.64), "C8_9": (2.54, 4.33), "C9_10": (2.53, 4.30)}
PAIRS = [(MOD_16APSK, r) for r in GAMMA_16] + [(MOD_32APSK, r) for r in GAMMA_32]

# (ring, angle) per label; rings counted from the inside (0 = R1). 16APSK angles in units of pi/12, 32APSK in units of pi/24.
_A16 = [(1, a) for a in (3, -3, 9, -9, 1, -1, 11, -11, 5, -5, 7, -7)] + [(0, a) for a in (3, -3, 9, -9)]
_A32 = ([(1, a) for a in (6, 10, -6, -10, 18, 14, -18, -14)] + [(2, a) for a in (3, 9, -6, -12, 18, 12, -21, -15)] +
        [(1, 2), (0, 6), (1, -2), (0, -6), (1, 22), (0, 18), (1, -22), (0, -18)] + [(2, a) for a in (0, 6, -3, -9, 21, 15, 24, -18)])


def radii(constellation, rate):
    if constellation == MOD_16APSK:
        g = GAMMA_16[rate]
        r1 = 2.0 / np.sqrt(1.0 + 3.0 * g * g)
        return (r1, g * r1)
    g1, g2 = GAMMA_32[rate]
    r1 = np.sqrt(32.0 / (4.0 + 12.0 * g1 * g1 + 16.0 * g2 * g2))
    return (r1, g1 * r1, g2 * r1)


def ring_angle(constellation):
    """[(ring, angle in radians)] by label"""
    if constellation == MOD_16APSK:
        return [(r, a * np.pi / 12) for r, a in _A16]
    return [(r, a * np.pi / 24) for r, a in _A32]


def points(constellation, rate):
    """complex128 table, entry i = label i, Es = 1"""
    rad = radii(constellation, rate)
    return np.array([rad[r] * (np.cos(a) + 1j * np.sin(a)) for r, a in ring_angle(constellation)], np.complex128)


def ring_walk(constellation, ring):
    """labels of one ring in the order of their angle"""
    ra = ring_angle(constellation)
    lab = [i for i, (r, _) in enumerate(ra) if r == ring]
    return sorted(lab, key=lambda i: np.mod(ra[i][1], 2 * np.pi))


def bits_of_labels(labels, n_mod):
    """(..., n_mod) bits, column 0 = most significant label bit"""
    return (np.asarray(labels)[..., None] >> np.arange(n_mod - 1, -1, -1)) & 1


def map_bits(cw_bits, pts):
    """Column interleaver of EN 302 307-1 5.3.2 (natural order) + mapper: codeword bits (nf, N) -> symbols (nf, N / n_mod)."""
    n_mod = int(np.log2(len(pts)))
    nf, N = cw_bits.shape
    rows = N // n_mod
    cols = cw_bits.reshape(nf, n_mod, rows).astype(np.int64)  # column c = bits c * rows .. (c + 1) * rows - 1
    labels = np.zeros((nf, rows), np.int64)
    for c in range(n_mod):
        labels |= cols[:, c, :] << (n_mod - 1 - c)
    return pts[labels]


def _n0_rows(n0, nf, dtype):
    n0 = np.atleast_1d(np.asarray(n0, np.float32))  # the kernel reads a float
    return (np.broadcast_to(n0, (nf,)) if n0.size == 1 else n0).astype(dtype)


def maxlog_f64(syms, n0, pts):
    """Brute-force max-log over all points in float64. syms (nf, rows) complex64 (exact in float64) -> L (nf, n_mod, rows)."""
    M = len(pts)
    n_mod = int(np.log2(M))
    y = np.asarray(syms).astype(np.complex128)
    nf = y.shape[0]
    d = np.abs(y[:, None, :] - np.asarray(pts, np.complex128)[None, :, None]) ** 2  # (nf, M, rows)
    b = bits_of_labels(np.arange(M), n_mod)  # (M, n_mod)
    out = np.empty((nf, n_mod, y.shape[1]))
    for c in range(n_mod):
        out[:, c, :] = d[:, b[:, c] == 1, :].min(axis=1) - d[:, b[:, c] == 0, :].min(axis=1)
    return out / _n0_rows(n0, nf, np.float64)[:, None, None], float(d.max())


def quantise(v):
    return np.clip(np.rint(v), -128, 127).astype(np.int8)


def demap_f64(syms, n0, pts):
    """(nf, n_llr) int8 in the frame layout"""
    L, _ = maxlog_f64(syms, n0, pts)
    return quantise(L).reshape(L.shape[0], -1)


def demap_f32(syms, n0, pts32):
    """The kernel's arithmetic in numpy float32, operation by operation (every line is one correctly rounded float operation per
    element, no fused multiply-add): dr = re - p.re; di = im - p.im; d = dr * dr + di * di; running minima per (column, bit value)
    over ALL points in label order; L = (min1 - min0) * (float)(1.0 / (double)N0); llr = sat8(rint(L)).
    pts32: complex64 table (the library's float table). Returns ((nf, n_llr) int8, L float32 (nf, n_mod, rows))."""
    pts32 = np.asarray(pts32, np.complex64)
    M = len(pts32)
    n_mod = int(np.log2(M))
    y = np.ascontiguousarray(syms, np.complex64)
    nf, rows = y.shape
    re, im = y.real.astype(np.float32), y.imag.astype(np.float32)
    inv = (1.0 / _n0_rows(n0, nf, np.float64)).astype(np.float32)
    m = np.full((2, n_mod, nf, rows), np.inf, np.float32)
    for i in range(M):
        dr = re - np.float32(pts32[i].real)
        di = im - np.float32(pts32[i].imag)
        d = dr * dr + di * di
        for c in range(n_mod):
            v = (i >> (n_mod - 1 - c)) & 1
            np.minimum(m[v, c], d, out=m[v, c])
    L = ((m[1] - m[0]) * inv[None, :, None]).transpose(1, 0, 2)
    assert L.dtype == np.float32
    return quantise(L).reshape(nf, -1), L


def snr_f64(syms, pts, ref_llr=None):
    """snr = sum |ref|^2 / sum |x - ref|^2 per frame in float64; ref = the nearest point, or the point whose label the signs of
    ref_llr (nf, n_mod * rows) spell through the column layout."""
    pts = np.asarray(pts, np.complex128)
    n_mod = int(np.log2(len(pts)))
    y = np.asarray(syms).astype(np.complex128)
    nf, rows = y.shape
    if ref_llr is None:
        lab = np.argmin(np.abs(y[:, None, :] - pts[None, :, None]), axis=1)
    else:
        b = (np.asarray(ref_llr).reshape(nf, n_mod, rows) < 0).astype(np.int64)
        lab = np.zeros((nf, rows), np.int64)
        for c in range(n_mod):
            lab |= b[:, c, :] << (n_mod - 1 - c)
    ref = pts[lab]
    return (np.abs(ref) ** 2).sum(axis=1) / np.maximum((np.abs(y - ref) ** 2).sum(axis=1), 1e-12)


# ---- the float32 / float64 quantisation bound (tests/test_apsk_model.py, notes/apsk_demap.md)
# u = 2^-24 is the unit roundoff of float32. With D the largest squared distance between a symbol of the set and a point:
#   table    each coordinate of a float point is off by <= u |s|, which moves one squared distance by <= 2 sqrt(D) u |s| <= 2 u D
#            (every |s|^2 <= D for these sets: the symbols lie around points of a ring and D spans the constellation)
#   distance dr and di carry one rounding each, their squares one more, the sum one: <= 4 u D
#   so each of the two minima is within 6 u D of its float64 value: 12 u D
#   the subtraction rounds once (<= u D), 1/N0 is rounded once and the product once (<= 2 u D): 15 u D in all, before / N0.
DELTA_CONST = 16.0


def delta_bound(d_max, n0):
    return DELTA_CONST * 2.0 ** -24 * d_max / float(np.min(np.atleast_1d(n0)))


def check_vs_f64(got, syms, n0, pts, what=""):
    """got (nf, n_llr) int8 may differ from the float64 model by one step and only where the float64 value lies within delta of a
    half-integer; the share of such LLRs may not exceed 4 delta. Returns (n_diff, delta, d_max)."""
    L, d_max = maxlog_f64(syms, n0, pts)
    nf = L.shape[0]
    delta = DELTA_CONST * 2.0 ** -24 * d_max / _n0_rows(n0, nf, np.float64)[:, None, None]
    want = quantise(L).reshape(nf, -1).astype(np.int32)
    got = np.asarray(got).astype(np.int32)
    diff = got != want
    frac = np.abs(L - np.floor(L) - 0.5).reshape(nf, -1)  # distance to the nearest half-integer
    near = frac <= np.broadcast_to(delta, L.shape).reshape(nf, -1)
    n_diff = int(diff.sum())
    print(f"{what}: {n_diff} of {diff.size} LLRs differ from float64, delta {float(delta.max()):.3e}, D_max {d_max:.3f}, "
          f"smallest distance of a differing value to a half-integer {frac[diff].min() if n_diff else float('nan'):.3e}")
    assert (np.abs(got - want)[diff] == 1).all(), what
    assert near[diff].all(), what
    assert n_diff <= 4.0 * float(delta.max()) * diff.size, what
    return n_diff, float(delta.max()), d_max
