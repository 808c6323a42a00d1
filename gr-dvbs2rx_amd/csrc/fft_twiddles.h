// fft_twiddles.h -- the ONE twiddle table of the library's radix-2 transforms (spectrum_hip.hip, pfbch_hip.hip): n / 2 entries
// (float(cos(2 pi i / n)), float(-sin(2 pi i / n))), evaluated in double and rounded once. Host code only. Internal, not installed.
#pragma once
#include <cmath>
#include <vector>

namespace dvbs2 {

// n a power of two >= 2; out: n / 2 (re, im) pairs. No checks: the callers have theirs
inline void fft_twiddles(int n, float* out)
{
    for (int i = 0; i < n / 2; i++) {
        const double x = 2.0 * M_PI * i / n;
        out[2 * i] = (float)std::cos(x);
        out[2 * i + 1] = (float)-std::sin(x);
    }
}

// The same entries in stage order, as the kernels read them: for stage s = 1..t its 2^(s-1) entries k 2^(t - s) of the table, k
// ascending, at 2^(s-1) - 1 + k; n - 1 pairs in a vector of n
inline std::vector<float> fft_twiddles_staged(int n, int t)
{
    std::vector<float> tw((size_t)n), staged(2 * (size_t)n, 0.0f);
    fft_twiddles(n, tw.data());
    for (int s = 1; s <= t; s++)
        for (int k = 0; k < 1 << (s - 1); k++) {
            const size_t to = (size_t)(1 << (s - 1)) - 1 + k, from = (size_t)k << (t - s);
            staged[2 * to] = tw[2 * from];
            staged[2 * to + 1] = tw[2 * from + 1];
        }
    return staged;
}

} // namespace dvbs2
