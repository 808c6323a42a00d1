// stdin rows -> one line each. Drives the host-only code of the pulse shaper (csrc/pulse_hip.hip: geometry, tap design, tap scaling, the
// argument check of the class) outside Python, so that it can be built with -fsanitize=address,undefined (rrc is csrc/rrc_pulse.h's, a
// header). Floats travel as the hexadecimal bits of a float32, so both directions are exact.
//   geom sps rrc_delay                      -> "ntaps history delay" or "refused"
//   taps sps rolloff rrc_delay tau gain     -> the taps, or "refused"
//   scale sps fullscale n tap ... tap       -> the scaled taps, or "refused"
//   check sps max_streams max_symbols n tap ... tap -> "ok" or "refused: <text>" (PulseShaperHip::check_args)
#include <iostream>
#include "../gr-dvbs2rx_amd/csrc/pulse_hip.h"
#include "host_main.h"

static void print_taps(const std::vector<float>& t)
{
    for (float f : t) std::printf("%08x ", to_bits(f));
    std::printf("\n");
}

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "geom") {
            int sps, delay, ntaps = -1, history = -1, d = -1;
            is >> sps >> delay;
            if (dvbs2::pulse_geometry(sps, delay, &ntaps, &history, &d)) std::printf("refused\n");
            else std::printf("%d %d %d\n", ntaps, history, d);
        } else if (what == "taps") {
            int sps, delay, ntaps = 0;
            double rolloff, tau, gain;
            is >> sps >> rolloff >> delay >> tau >> gain;
            if (dvbs2::pulse_geometry(sps, delay, &ntaps, nullptr, nullptr)) { std::printf("refused\n"); continue; }
            std::vector<float> t(ntaps);
            if (dvbs2::pulse_taps(sps, (float)rolloff, delay, tau, gain, t.data())) std::printf("refused\n");
            else print_taps(t);
        } else if (what == "scale") {
            int sps, n;
            double fullscale;
            is >> sps >> fullscale >> n;
            std::vector<float> t = read_taps(is, n);
            if (dvbs2::pulse_scale_taps(t.empty() ? nullptr : t.data(), n, sps, fullscale)) std::printf("refused\n");
            else print_taps(t);
        } else if (what == "check") {
            int sps, max_streams, max_symbols, n;
            is >> sps >> max_streams >> max_symbols >> n;
            const std::vector<float> t = read_taps(is, n);
            const std::string bad = dvbs2::PulseShaperHip::check_args(sps, t.empty() ? nullptr : t.data(), n, max_streams, max_symbols);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
