// stdin rows -> one line each. Drives the host-only code of the digital down-converter (csrc/ddc_hip.hip: geometry, the count rule, the
// tile rule, the counter and phase mirror over a sequence of calls, the argument check of the class) outside Python, so that it can be
// built with -fsanitize=address,undefined. Floats travel as the hexadecimal bits of a float32, so both directions are exact.
//   geom decim ntaps                          -> "history delay_num" or "refused"
//   produce position decim n_in               -> "n" or "refused"
//   tile decim ntaps                          -> "tile"
//   mirror decim nch inc ... inc k (n_in n_channels) ... -> "n_out counter phase ... phase" per call, counter and phases carried over
//   check decim max_channels max_inputs max_samples n tap ... tap -> "ok" or "refused: <text>" (DdcHip::check_args)
#include <cstdlib>
#include <iostream>
#include "../gr-dvbs2rx_amd/csrc/ddc_hip.h"
#include "host_main.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "geom") {
            int decim, ntaps, history = -1, delay = -1;
            is >> decim >> ntaps;
            if (dvbs2::ddc_geometry(decim, ntaps, &history, &delay)) std::printf("refused\n");
            else std::printf("%d %d\n", history, delay);
        } else if (what == "produce") {
            long long position;
            int decim, n_in;
            is >> position >> decim >> n_in;
            const int64_t n = dvbs2::ddc_produce(position, decim, n_in);
            if (n < 0) std::printf("refused\n");
            else std::printf("%lld\n", (long long)n);
        } else if (what == "tile") {
            int decim, ntaps;
            is >> decim >> ntaps;
            std::printf("%d\n", dvbs2::ddc_tile(decim, ntaps));
        } else if (what == "mirror") {
            int decim, nch, k;
            is >> decim >> nch;
            dvbs2::DdcMirror m;
            m.phase.assign((size_t)nch, 0);
            for (int c = 0; c < nch; c++) { unsigned long long inc; is >> inc; m.inc.push_back(inc); }
            is >> k;
            for (int i = 0; i < k; i++) {
                int n_in, n_channels;
                is >> n_in >> n_channels;
                std::printf("%lld ", (long long)dvbs2::ddc_produce(m.counter, decim, n_in));
                m.advance(n_in, n_channels);
                std::printf("%lld ", (long long)m.counter);
                for (int c = 0; c < nch; c++) std::printf("%llu ", (unsigned long long)m.phase[c]);
            }
            std::printf("\n");
        } else if (what == "check") {
            int decim, max_channels, max_inputs, max_samples, n;
            is >> decim >> max_channels >> max_inputs >> max_samples >> n;
            const std::vector<float> t = read_taps(is, n);
            const std::string bad = dvbs2::DdcHip::check_args(decim, t.empty() ? nullptr : t.data(), n, max_channels, max_inputs, max_samples);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
