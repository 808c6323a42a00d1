// stdin rows -> one line each. Drives the host-only code of the resampler (csrc/resamp_hip.hip: step, geometry, max_out, the position rule
// over a sequence of calls, the argument check of the class) outside Python, so that it can be built with -fsanitize=address,undefined.
// Floats travel as the hexadecimal bits of a float32, the rate as a C99 hexadecimal double, so both directions are exact.
//   step rate                                -> "step" or "refused"
//   geom nfilts ntaps                        -> "L history delay_num" or "refused"
//   maxout step n_in                         -> "n" or "refused"
//   produce step acc k n_in ... n_in         -> "n_out acc'" per call, acc carried over
//   check nfilts rate max_streams max_samples n tap ... tap -> "ok" or "refused: <text>" (ResamplerHip::check_args)
#include <cstdlib>
#include <iostream>
#include "../gr-dvbs2rx_amd/csrc/resamp_hip.h"
#include "host_main.h"

static double read_double(std::istringstream& is)
{
    std::string s;
    is >> s;
    return std::strtod(s.c_str(), nullptr); // hexadecimal doubles, nan and inf included
}

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "step") {
            uint64_t step = 0;
            if (dvbs2::resamp_step(read_double(is), &step)) std::printf("refused\n");
            else std::printf("%llu\n", (unsigned long long)step);
        } else if (what == "geom") {
            int nfilts, ntaps, L = -1, history = -1, delay = -1;
            is >> nfilts >> ntaps;
            if (dvbs2::resamp_geometry(nfilts, ntaps, &L, &history, &delay)) std::printf("refused\n");
            else std::printf("%d %d %d\n", L, history, delay);
        } else if (what == "maxout") {
            unsigned long long step;
            int n_in;
            is >> step >> n_in;
            const int64_t n = dvbs2::resamp_max_out(step, n_in);
            if (n < 0) std::printf("refused\n");
            else std::printf("%lld\n", (long long)n);
        } else if (what == "produce") {
            unsigned long long step, acc0;
            int k;
            is >> step >> acc0 >> k;
            uint64_t acc = acc0;
            for (int c = 0; c < k; c++) {
                int n_in;
                is >> n_in;
                const int64_t n = dvbs2::resamp_advance(acc, step, n_in, &acc);
                std::printf("%lld %llu ", (long long)n, (unsigned long long)acc);
            }
            std::printf("\n");
        } else if (what == "check") {
            int nfilts, max_streams, max_samples, n;
            is >> nfilts;
            const double rate = read_double(is);
            is >> max_streams >> max_samples >> n;
            const std::vector<float> t = read_taps(is, n);
            const std::string bad = dvbs2::ResamplerHip::check_args(nfilts, t.empty() ? nullptr : t.data(), n, rate, max_streams, max_samples);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
