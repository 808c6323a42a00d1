// awgn_math.hpp -- the arithmetic of the AWGN channel stage (awgn_hip.h), shared by the kernel and the host restatement
// (dvbs2_awgn_words / dvbs2_awgn_sample) and restated once more in numpy float32 by tests/awgn_model.py; the three agree bit for bit.
// The noise of complex sample n (>= 0) of stream s under seed k is a pure function of (k, s, n):
//   words      Philox4x32-10 (Salmon et al., SC'11; the constants of Random123), counter (lo32(n >> 1), hi32(n >> 1), lo32(s), hi32(s)),
//              key (lo32(k), hi32(k)); sample n takes words (w0, w1) when n is even and (w2, w3) when it is odd: wa, wb
//   transform  Box-Muller of u1 = (wa + 1/2) 2^-32, u2 = (wb + 1/2) 2^-32: radius r = sqrt(-2 ln u1), noise (r cos, r sin)(2 pi u2),
//              built from integer steps and float32 polynomials (below), no libm call but the correctly rounded sqrtf
//   channel    y = x + sigma * noise per component, one product then one addition; without an input the product alone
// Every float step is one IEEE float32 operation in the written order; the file is built with -ffp-contract=off and says so itself.
// Coefficients, their source (tools/awgn_fit.py), the errors and the bound against float64: notes/awgn.md.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AWGN_HD __host__ __device__ inline
#else
#define AWGN_HD inline
#endif

#pragma clang fp contract(off)

namespace dvbs2 {

struct AwgnWords { uint32_t w[4]; };
struct AwgnPair { float re, im; };

AWGN_HD AwgnWords awgn_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return AwgnWords{ { c0, c1, c2, c3 } };
}

// the generator block that holds samples 2 b and 2 b + 1 of stream s
AWGN_HD AwgnWords awgn_block(uint64_t seed, uint64_t stream_id, uint64_t b)
{
    return awgn_philox((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

AWGN_HD float awgn_float_of_bits(uint32_t b) { return __builtin_bit_cast(float, b); }
static_assert(__builtin_bit_cast(uint32_t, 1.41421354f) == 0x3FB504F3u && __builtin_bit_cast(uint32_t, 0.693147182f) == 0x3F317218u &&
              __builtin_bit_cast(uint32_t, 4.6813379839250047e-08f) == 0x33490FDBu, "the literals below are these float32 values");

// r = sqrt(-2 ln u1), u1 = (2 wa + 1) 2^-33. v = 2 wa + 1 has its top bit at e; its top 24 bits, truncated, are the float m in [1, 2);
// above sqrt 2 it is halved (e + 1), so f = m - 1 is exact and lies in (1/sqrt 2 - 1, sqrt 2 - 1]; -ln u1 ~ t = (33 - e) ln 2 - log1p(f) > 0:
// with e = 33 f is negative (at most -2^-24) and the polynomial below is then negative, else t >= ln 2 - log1p(sqrt 2 - 1) = 0.34.
AWGN_HD float awgn_radius(uint32_t wa)
{
    const uint64_t v = 2 * (uint64_t)wa + 1;
    int e = 63 - __builtin_clzll(v);
    const uint32_t top = (uint32_t)(e >= 23 ? v >> (e - 23) : v << (23 - e)); // in [2^23, 2^24)
    float m = awgn_float_of_bits(0x3F800000u | (top & 0x7FFFFFu));
    if (m > 1.41421354f) { m = m * 0.5f; e = e + 1; }
    const float f = m - 1.0f;
    float q = 0.08733489364385605f;
    q = q * f + -0.14441822469234467f;
    q = q * f + 0.1497931331396103f;
    q = q * f + -0.1655234396457672f;
    q = q * f + 0.19953611493110657f;
    q = q * f + -0.2500249147415161f;
    q = q * f + 0.3333422541618347f;
    q = q * f + -0.4999998211860657f;
    const float ff = f * f;
    const float l = f + ff * q;
    const float t = (float)(33 - e) * 0.693147182f - l;
    return sqrtf(2.0f * t);
}

// (cos, sin)(2 pi u2), u2 = (wb + 1/2) 2^-32 with the low 6 bits of wb left out: the top 3 bits are the octant, the next 23 with a one
// behind them the odd 24-bit position p inside it (mirrored, 2^24 - p, in the odd octants, where the angle runs back from the next
// axis), a = p * (pi/4 2^-24) in (0, pi/4). One sine and one cosine there, then swapped and negated by octant.
AWGN_HD AwgnPair awgn_angle(uint32_t wb)
{
    const uint32_t oct = wb >> 29;
    uint32_t p = ((wb >> 5) & 0xFFFFFEu) | 1u;
    if (oct & 1u) p = 0x1000000u - p;
    const float a = (float)p * 4.6813379839250047e-08f; // fl(pi/4) 2^-24, bits 0x33490FDB
    const float z = a * a;
    float s = -0.000194956359337084f;
    s = s * z + 0.00833197869360447f;
    s = s * z + -0.16666650772094727f;
    const float az = a * z;
    const float sn = a + az * s;
    float c = 2.4390452381339855e-05f;
    c = c * z + -0.0013886763481423259f;
    c = c * z + 0.04166662320494652f;
    c = c * z + -0.5f;
    const float cs = 1.0f + z * c;
    const bool swap = ((oct + 1u) >> 1) & 1u; // octants 1, 2, 5, 6
    float x = swap ? sn : cs, y = swap ? cs : sn;
    if (((oct + 2u) >> 2) & 1u) x = -x; // octants 2..5
    if (oct >> 2) y = -y;               // octants 4..7
    return AwgnPair{ x, y };
}

AWGN_HD AwgnPair awgn_noise(uint32_t wa, uint32_t wb)
{
    const float r = awgn_radius(wa);
    const AwgnPair d = awgn_angle(wb);
    return AwgnPair{ r * d.re, r * d.im };
}

AWGN_HD AwgnPair awgn_channel(AwgnPair x, float sigma, AwgnPair noise) { return AwgnPair{ x.re + sigma * noise.re, x.im + sigma * noise.im }; }
AWGN_HD AwgnPair awgn_channel(float sigma, AwgnPair noise) { return AwgnPair{ sigma * noise.re, sigma * noise.im }; }

// host conveniences: the words (wa, wb) and the unit-variance noise of one sample
AWGN_HD void awgn_words_of(uint64_t seed, uint64_t stream_id, int64_t index, uint32_t* wa, uint32_t* wb)
{
    const AwgnWords w = awgn_block(seed, stream_id, (uint64_t)index >> 1);
    *wa = w.w[(index & 1) * 2]; *wb = w.w[(index & 1) * 2 + 1];
}

} // namespace dvbs2
