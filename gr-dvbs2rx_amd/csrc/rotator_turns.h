// rotator_turns.h -- a phase increment in radians as 64-bit fixed-point turns: the one conversion behind the rotator (rotator_hip.hip)
// and the mixer of the down-converter (ddc_hip.hip). Host only, plain C++, no HIP header.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

namespace dvbs2 {

#ifndef __HIP_DEVICE_COMPILE__ // host code only: the device pass of a kernel unit has no extended type and never runs this
static_assert(LDBL_MANT_DIG >= 64, "the increment is converted with a 64-bit significand");
#endif

// inc (radians per sample, any finite value) as turns in 2^-64 units, reduced modulo one turn
inline uint64_t rotator_inc_turns(double inc)
{
    // 2 pi to a 64-bit significand; the quotient is within 2^-63 (relative) of inc / 2 pi, then rounded to 2^-64 turns
    const long double two_pi = 6.283185307179586476925286766559005768L;
    long double t = (long double)inc / two_pi;
    t -= floorl(t); // [0, 1]
    const long double s = roundl(ldexpl(t, 64));
    if (s >= 0x1p64L) return 0;
    return (uint64_t)s;
}

} // namespace dvbs2
