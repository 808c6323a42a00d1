#!/usr/bin/env python3
"""Where the polynomial coefficients of csrc/awgn_math.hpp come from, and the error figures notes/awgn.md quotes for them. CPU only.

Three float32 polynomials, each a weighted least-squares fit on Chebyshev nodes whose weights are moved towards the equal-ripple
(minimax) solution by Lawson's iteration, with the coefficients then rounded to float32:
  log1p(f) ~ f + f^2 Q(f)          f in [1/sqrt 2 - 1, sqrt 2 - 1],  Q of degree 7
  sin(a)   ~ a + (a z) S(z)        a in (0, pi/4), z = a^2,          S of degree 2
  cos(a)   ~ 1 + z C(z)                                              C of degree 3
For each it prints the rounded coefficients (decimal and the bits), the largest error of the ROUNDED polynomial in exact arithmetic
(float64 on a dense grid) and an a-priori bound for its float32 evaluation in the order the header writes: the last addition
rounds once (u |value|) and the correction term carries at most k roundings, gamma_k = k u / (1 - k u) times the sum of the absolute
values of its terms at the far end of the interval. Nothing here looks at the generator's output."""
import numpy as np

U = 2.0 ** -24


def nodes(a, b, n=20001):
    k = np.arange(n)
    return 0.5 * (a + b) + 0.5 * (b - a) * np.cos(np.pi * (k + 0.5) / n)


def lawson(x, target, weight, deg, iters=30):
    w = np.ones_like(x)
    for _ in range(iters):
        v = np.vander(x, deg + 1, increasing=True) * (weight * w)[:, None]
        c = np.linalg.lstsq(v, target * weight * w, rcond=None)[0]
        err = np.abs((np.polyval(c[::-1], x) - target) * weight)
        w = w * (0.5 + err / err.max())
        w /= w.max()
    return c.astype(np.float32)


def gamma(k):
    return k * U / (1 - k * U)


def show(name, c, approx, evalb):
    print(f"{name}: " + ", ".join(f"{float(v)!r}f" for v in c))
    print("   bits " + " ".join(f"{b:08x}" for b in c.view(np.uint32)))
    print(f"   approximation {approx:.3e}   evaluation {evalb:.3e}")


def main():
    lo, hi = 1 / np.sqrt(2) - 1, np.sqrt(2) - 1
    f = nodes(lo, hi)
    f = f[np.abs(f) > 1e-6]
    q = lawson(f, (np.log1p(f) - f) / f ** 2, f ** 2, 7)
    q64 = q.astype(np.float64)
    approx = np.abs(f + f * f * np.polyval(q64[::-1], f) - np.log1p(f)).max()
    # f*f, Horner of degree 7 (14 roundings), the product: 16 roundings on the correction; then one addition
    evalb = U * np.log1p(hi) + gamma(16) * hi * hi * np.polyval(np.abs(q64)[::-1], hi)
    show("log1p Q", q, approx, evalb)

    a = nodes(0.0, np.pi / 4)
    a = a[a > 1e-4]
    z = a * a
    zmax = (np.pi / 4) ** 2
    s = lawson(z, (np.sin(a) / a - 1) / z, a * z, 2)
    s64 = s.astype(np.float64)
    approx = np.abs(a + a * z * np.polyval(s64[::-1], z) - np.sin(a)).max()
    # z, a*z, Horner of degree 2 (4), the product: 7 roundings on the correction (z counts twice); then one addition
    evalb = U * np.sin(np.pi / 4) + gamma(8) * (np.pi / 4) * zmax * np.polyval(np.abs(s64)[::-1], zmax)
    show("sin S", s, approx, evalb)

    c = lawson(z, (np.cos(a) - 1) / z, z, 3)
    c64 = c.astype(np.float64)
    approx = np.abs(1 + z * np.polyval(c64[::-1], z) - np.cos(a)).max()
    # z, Horner of degree 3 (6, z in each), the product: at most 11 roundings on the correction; then one addition (the sum is <= 1)
    evalb = U * 1.0 + gamma(11) * zmax * np.polyval(np.abs(c64)[::-1], zmax)
    show("cos C", c, approx, evalb)


if __name__ == "__main__":
    main()
