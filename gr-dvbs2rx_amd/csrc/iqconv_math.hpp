// iqconv_math.hpp -- the arithmetic of the IQ sample converter (iqconv_hip.h), shared by the kernels and the host restatement
// (dvbs2_iqconv_unpack_host / dvbs2_iqconv_pack_host) and restated once more in numpy float32 by tests/iqconv_model.py; the three agree
// bit for bit. One complex sample is the I code, then the Q code; a component is converted on its own. Per format, with bias B, full
// scale F and the code range [lo, hi]:
//              B      F      lo      hi     middle code
//   u8       127.5    128       0     255   128
//   s8         0      128    -128     127     0
//   s16        0    32768  -32768   32767     0
//   unpack   y = (float(c) - B) / F * gain. (float(c) - B) / F is exact for every code, and gain lies in [2^-64, 2^64], so gain / F is
//            exact as well: the kernel forms (float(c) - B) * (gain / F), ONE rounded float32 product, the float32 nearest to the real
//            number (c - B) / F * gain. With gain == 1 nothing is rounded: the reference's receive chain (apps/dvbs2-rx:685-707).
//   pack     t = x * gain (one product); u = t * F (a power of two: exact unless it overflows to infinity, which then saturates);
//            w = u + B (one addition; nothing when B == 0); r = w rounded to the nearest integer, ties to even; the code is r clamped
//            to [lo, hi]; a NaN gives the middle code. With gain == 1 and u8 this is the wiring of apps/dvbs2-tx:535-542
//            (multiply_const 128, add_const 127.5, float_to_uchar), taking float_to_uchar as rint plus clamp. GNU Radio is not in the
//            reference tree: the stage is UNPINNED against it.
//   level    d = 2 c - 255 for u8 (units of 1/256 of full scale), d = c for the signed formats; energy sums d * d, an exact integer.
//   clipped  unpack: the code sits on a rail (lo or hi), which is how a saturated ADC reads. pack: r < lo, r > hi or NaN; a value
//            that merely rounds onto the rail does not count.
// sqrt(energy / samples) / (256 or F) is the block-mean form of the reading blocks.rms_cf gives the reference's GUI
// (apps/dvbs2-rx:952); rms_cf itself, a one-pole IIR, is not restated.
// Every float step is one IEEE float32 operation in the written order, denormals kept; the file is built with -ffp-contract=off and
// says so itself.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IQCONV_HD __host__ __device__ inline
#else
#define IQCONV_HD inline
#endif

#pragma clang fp contract(off)

namespace dvbs2 {

enum IqFormatId { kIqU8 = 0, kIqS8 = 1, kIqS16 = 2 };

template <int kFmt> struct IqFormat;
template <> struct IqFormat<kIqU8> {
    static constexpr float bias = 127.5f, full = 128.0f;
    static constexpr int lo = 0, hi = 255, mid = 128, bytes = 1;
};
template <> struct IqFormat<kIqS8> {
    static constexpr float bias = 0.0f, full = 128.0f;
    static constexpr int lo = -128, hi = 127, mid = 0, bytes = 1;
};
template <> struct IqFormat<kIqS16> {
    static constexpr float bias = 0.0f, full = 32768.0f;
    static constexpr int lo = -32768, hi = 32767, mid = 0, bytes = 2;
};

constexpr float kIqGainMin = 5.42101086e-20f, kIqGainMax = 1.84467441e+19f; // 2^-64 and 2^64
static_assert(__builtin_bit_cast(uint32_t, kIqGainMin) == 0x1F800000u && __builtin_bit_cast(uint32_t, kIqGainMax) == 0x5F800000u,
              "the literals above are these powers of two");

// gain / F: exact for a gain the stage accepts
template <int kFmt> IQCONV_HD float iq_unpack_scale(float gain) { return gain * (1.0f / IqFormat<kFmt>::full); }

template <int kFmt> IQCONV_HD float iq_unpack(int c, float scale)
{
    if constexpr (IqFormat<kFmt>::bias != 0.0f) return ((float)c - IqFormat<kFmt>::bias) * scale;
    else return (float)c * scale;
}

// the code of x; *clipped: the rounded value lay outside [lo, hi], or x * gain was a NaN
template <int kFmt> IQCONV_HD int iq_pack(float x, float gain, bool* clipped)
{
    using F = IqFormat<kFmt>;
    const float t = x * gain;
    float w = t * F::full;
    if constexpr (F::bias != 0.0f) w = w + F::bias;
    const float r = rintf(w); // the default rounding mode: to nearest, ties to even
    const bool nan = r != r, below = r < (float)F::lo, above = r > (float)F::hi;
    *clipped = nan || below || above;
    return nan ? F::mid : below ? F::lo : above ? F::hi : (int)r;
}

template <int kFmt> IQCONV_HD int iq_level(int c) { return kFmt == kIqU8 ? 2 * c - 255 : c; }
template <int kFmt> IQCONV_HD bool iq_on_rail(int c) { return c == IqFormat<kFmt>::lo || c == IqFormat<kFmt>::hi; }

} // namespace dvbs2
