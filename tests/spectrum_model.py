"""The spectrum stage restated (include/dvbs2_fec_hip.h, dvbs2_spectrum_*): (a) the device's arithmetic in numpy float32, operation by
operation -- window product, the radix-2 decimation-in-time graph over the library's one twiddle table, the power, the two-level sum
and the scale -- which the device equals bit for bit; (b) the same spectrum in float64 with the error bound of (a) against it; (c) the
carrier finder in double, operation by operation. numpy's float32 products and sums are IEEE single operations, nothing fused."""
import math

import numpy as np

CHUNK = 16  # DVBS2_SPECTRUM_CHUNK
U = 2.0 ** -24  # unit roundoff of float32
F = np.float32
DEFAULTS = dict(smooth=9, floor_quantile=0.25, threshold_db=6.0, min_gap=4, min_width=8)


# ------------------------------------------------------------------ counts, windows, table
def geometry(nfft, hop, avg, n_in):
    """(n_seg, n_rows, used_samples) in plain Python integers"""
    n_seg = (n_in - nfft) // hop + 1 if n_in >= nfft else 0
    n_rows = n_seg // avg if avg > 0 else (1 if n_seg > 0 else 0)
    used = n_rows * avg if avg > 0 else n_seg
    return n_seg, n_rows, ((used - 1) * hop + nfft if used > 0 else 0)


def window64(kind, nfft):
    """the periodic windows in float64"""
    x = 2.0 * np.pi * np.arange(nfft) / nfft
    if kind == "rect":
        return np.ones(nfft)
    if kind == "hann":
        return 0.5 - 0.5 * np.cos(x)
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(x)
    if kind == "blackman-harris":
        return 0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)
    raise ValueError(kind)


def twiddles64(nfft):
    x = 2.0 * np.pi * np.arange(nfft // 2) / nfft
    return np.cos(x) - 1j * np.sin(x)


def window_power(w):
    """sum w[n]^2 in double, ascending n (cumsum adds in order)"""
    return float(np.cumsum(np.asarray(w, F).astype(np.float64) ** 2)[-1])


def bitrev(nfft):
    t = nfft.bit_length() - 1
    i = np.arange(nfft)
    r = np.zeros(nfft, np.int64)
    for b in range(t):
        r |= ((i >> b) & 1) << (t - 1 - b)
    return r


# ------------------------------------------------------------------ (a) the device's arithmetic
def fft32(xw_re, xw_im, table):
    """The transform of the windowed segments [..., nfft] (float32 real and imaginary parts) over `table` (complex64 [nfft / 2], the
    library's). Returns (Xr, Xi) float32."""
    nfft = xw_re.shape[-1]
    t = nfft.bit_length() - 1
    rev = bitrev(nfft)
    re, im = np.ascontiguousarray(xw_re[..., rev], F), np.ascontiguousarray(xw_im[..., rev], F)  # place i holds sample bitrev(i)
    wr_all, wi_all = np.ascontiguousarray(table.real, F), np.ascontiguousarray(table.imag, F)
    lead = re.shape[:-1]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s in range(1, t + 1):
            half = 1 << (s - 1)
            re, im = re.reshape(lead + (nfft >> s, 2, half)), im.reshape(lead + (nfft >> s, 2, half))
            ar, ai, br, bi = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
            if s == 1:
                tr, ti = br, bi
            else:
                k = np.arange(half) * (nfft >> s)
                wr, wi = wr_all[k], wi_all[k]
                tr = wr * br - wi * bi
                ti = wr * bi + wi * br
            re = np.stack([ar + tr, ar - tr], axis=-2).reshape(lead + (nfft,))
            im = np.stack([ai + ti, ai - ti], axis=-2).reshape(lead + (nfft,))
    return re, im


def segments(x, nfft, hop, n_seg):
    i = np.arange(n_seg)[:, None] * hop + np.arange(nfft)[None, :]
    return x[i]


def rows32(x, nfft, hop, avg, window, table, shifted):
    """The rows of one stream x (complex64) as float32 [n_rows, nfft], the device's bits."""
    x = np.asarray(x, np.complex64)
    w = np.asarray(window, F)
    n_seg, n_rows, _ = geometry(nfft, hop, avg, x.size)
    if n_rows == 0:
        return np.zeros((0, nfft), F)
    per_row = avg if avg > 0 else n_seg
    seg = segments(x, nfft, hop, n_rows * per_row)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xr, xi = fft32(seg.real * w, seg.imag * w, table)
        p = (xr * xr + xi * xi).reshape(n_rows, per_row, nfft)
        out = np.zeros((n_rows, nfft), F)
        for c0 in range(0, per_row, CHUNK):
            chunk = np.zeros((n_rows, nfft), F)
            for s in range(c0, min(c0 + CHUNK, per_row)):
                chunk = chunk + p[:, s]
            out = out + chunk
        scale = F(1.0 / (per_row * window_power(w)))
        out = out * scale
    return np.fft.fftshift(out, axes=-1) if shifted else out


# ------------------------------------------------------------------ (b) float64 and the bound
def gamma(n):
    return n * U / (1.0 - n * U)


def fft_eta(table, nfft):
    """eta of Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2: mu + gamma_4 (sqrt 2 + mu), mu the table's largest
    absolute error"""
    mu = float(np.abs(table.astype(np.complex128) - twiddles64(nfft)).max())
    return mu + gamma(4) * (math.sqrt(2.0) + mu), mu


def rows64(x, nfft, hop, avg, window, table, shifted):
    """(rows in float64 from numpy.fft.fft of the float64-windowed input, the bound of |rows32 - rows64| per element). The window is
    the float32 window the device holds, taken as exact. notes/spectrum.md derives the bound:
      transform   ||X^ - X||_2 <= ((1 + u)(1 + B) - 1) ||X||_2 =: E ||X||_2, B = t eta / (1 - t eta), u from the window product;
                  every |X^[k] - X[k]| <= E ||X||_2 =: d
      power       |p^ - p| <= (2 |X[k]| d + d^2)(1 + gamma_2) + gamma_2 |X[k]|^2
      sums        a sum of n terms in two levels is off by at most gamma_{16 + ceil(n / 16)} sum |terms|
      scale       two more roundings (the scale's own and the product's)"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    w = np.asarray(window, F).astype(np.float64)
    n_seg, n_rows, _ = geometry(nfft, hop, avg, x.size)
    per_row = avg if avg > 0 else n_seg
    seg = segments(x, nfft, hop, n_rows * per_row) * w
    X = np.fft.fft(seg, axis=-1)
    t = nfft.bit_length() - 1
    eta, _ = fft_eta(table, nfft)
    E = (1.0 + U) * (1.0 + t * eta / (1.0 - t * eta)) - 1.0
    d = E * np.sqrt((np.abs(X) ** 2).sum(axis=-1, keepdims=True))
    p = np.abs(X) ** 2
    dp = (2.0 * np.abs(X) * d + d * d) * (1.0 + gamma(2)) + gamma(2) * p
    g_sum = gamma(CHUNK + (per_row + CHUNK - 1) // CHUNK)
    p, dp = p.reshape(n_rows, per_row, nfft), dp.reshape(n_rows, per_row, nfft)
    s = 1.0 / (per_row * (w * w).sum())
    rows = p.sum(axis=1) * s
    bound = (dp.sum(axis=1) * (1.0 + g_sum) + g_sum * p.sum(axis=1)) * s * (1.0 + gamma(3)) + gamma(3) * rows + 2.0 ** -149
    if shifted:
        rows, bound = np.fft.fftshift(rows, axes=-1), np.fft.fftshift(bound, axes=-1)
    return rows, bound


# ------------------------------------------------------------------ (c) the carrier finder
def carriers(psd, shifted, smooth=9, floor_quantile=0.25, threshold_db=6.0, min_gap=4, min_width=8):
    """csrc/spectrum_carriers.cpp in Python: a list of dicts (centre, bandwidth, level, floor, lo_bin, hi_bin) sorted by centre."""
    y = np.asarray(psd, F).astype(np.float64)
    N = y.size
    rot = 0 if shifted else N // 2
    y = np.roll(y, -rot)  # y[i] = psd[(i + rot) mod N]
    h = (smooth - 1) // 2
    acc = np.zeros(N)
    for d in range(-h, h + 1):
        acc = acc + np.roll(y, -d)  # y[(i + d) mod N], d ascending
    sm = acc / smooth
    floor = float(np.sort(sm)[int(math.floor(floor_quantile * (N - 1)))])
    thr = floor * math.pow(10.0, threshold_db / 10.0)
    up = sm > thr
    best_start, best_len = -1, 0
    for i in range(N):
        if up[i] or not up[i - 1]:
            continue
        n = 1
        while n < N and not up[(i + n) % N]:
            n += 1
        if n > best_len:
            best_len, best_start = n, i
    if best_start < 0 or best_len < min_gap:
        return []
    u, end, regions = best_start + best_len, best_start + N, []
    while u < end:
        if not up[u % N]:
            u += 1
            continue
        b = u
        while b < end and up[b % N]:
            b += 1
        if regions and u - regions[-1][1] < min_gap:
            regions[-1][1] = b
        else:
            regions.append([u, b])
        u = b
    found = []
    def e(u):
        return float(sm[u % N]) - floor

    for r, (a, b) in enumerate(regions):
        w = b - a
        if w < min_width:
            continue
        before = regions[r - 1][1] if r > 0 else regions[-1][1] - N
        behind = regions[r + 1][0] if r + 1 < len(regions) else regions[0][0] + N
        lo_limit, hi_limit = a - (a - before) // 2, b + (behind - b) // 2
        ca, cb = a, b
        while ca > lo_limit and e(ca - 1) > 0.0:
            ca -= 1
        while cb < hi_limit and e(cb) > 0.0:
            cb += 1
        se = su = 0.0
        for u in range(ca, cb):
            se += e(u)
            su += e(u) * float(u)
        m0, m1 = a + w // 4, b - w // 4
        mid = sorted(e(u) for u in range(m0, m1))
        k = len(mid)
        level = mid[k // 2] if k & 1 else 0.5 * (mid[k // 2 - 1] + mid[k // 2])
        half = 0.5 * level
        xl, xr = float(a), float(b)
        if level > 0.0:
            u = m0
            while u > m0 - N and e(u) >= half:
                u -= 1
            v = m1 - 1
            while v < m1 - 1 + N and e(v) >= half:
                v += 1
            if e(u) < half and e(v) < half:
                xl = u + (half - e(u)) / (e(u + 1) - e(u))
                xr = v - (half - e(v)) / (e(v - 1) - e(v))
        f = (su / se) / N - 0.5
        f -= math.floor(f + 0.5)
        found.append(dict(centre=f, bandwidth=(xr - xl) / N, level=level, floor=floor, lo_bin=(a + rot) % N, hi_bin=(b - 1 + rot) % N))
    return sorted(found, key=lambda c: c["centre"])


def raised_cosine_psd(nfft, centre, rs, rolloff, level, floor):
    """An exact row in shifted order: a raised cosine of symbol rate rs (cycles per sample) around `centre` on a flat floor; circular."""
    f = (np.arange(nfft) - nfft // 2) / nfft
    d = np.abs((f - centre + 0.5) % 1.0 - 0.5) / rs
    lo, hi = (1 - rolloff) / 2, (1 + rolloff) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        edge = 0.5 * (1 + np.cos(np.pi / rolloff * (d - lo))) if rolloff > 0 else np.zeros(nfft)
    shape = np.where(d <= lo, 1.0, np.where(d < hi, edge, 0.0))
    return (floor + level * shape).astype(F)
