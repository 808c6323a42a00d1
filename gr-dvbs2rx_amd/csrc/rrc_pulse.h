// rrc_pulse.h -- the root raised cosine in closed form: the one prototype behind symsync_taps (symsync_hip.hip) and pulse_taps
// (pulse_hip.hip). Host only, plain C++, no HIP header.
#pragma once
#include <cmath>

namespace dvbs2 {

// the RRC impulse response at t symbols (unit symbol rate, rolloff a in [0, 1]); the two singular points by their limits
inline double rrc(double t, double a)
{
#pragma clang fp contract(off) // the tap values are pinned: every product and sum rounded on its own (the library is built -ffp-contract=off as well)
    const double pi = M_PI;
    if (t == 0.0) return 1.0 - a + 4.0 * a / pi;
    if (a > 0.0 && fabs(fabs(4.0 * a * t) - 1.0) < 1e-9)
        return a / sqrt(2.0) * ((1.0 + 2.0 / pi) * sin(pi / (4.0 * a)) + (1.0 - 2.0 / pi) * cos(pi / (4.0 * a)));
    return (sin(pi * t * (1.0 - a)) + 4.0 * a * t * cos(pi * t * (1.0 + a))) / (pi * t * (1.0 - 16.0 * a * a * t * t));
}

} // namespace dvbs2
