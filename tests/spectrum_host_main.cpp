// stdin rows -> one line each. Drives the host-only code of the spectrum stage (csrc/spectrum_hip.hip: geometry, windows, the twiddle
// table, the argument check of the class; csrc/spectrum_carriers.cpp: the carrier finder) outside Python, so that it can be built with
// -fsanitize=address,undefined. Floats travel as the hexadecimal bits of a float32, doubles as those of a float64: exact both ways.
//   geom nfft hop avg n_in                     -> "n_seg n_rows used_samples" or "refused"
//   window kind nfft                           -> nfft floats, or "refused"
//   twiddles nfft                              -> nfft floats (re, im pairs), or "refused"
//   check nfft hop avg max_streams max_samples n w ... w   -> "ok" or "refused: <text>" (SpectrumHip::check_args; n == 0: null window)
//   carriers shifted smooth quantile threshold_db min_gap min_width nfft p ... p
//                                              -> "k" then per carrier "centre bandwidth level floor lo hi", or "refused: <text>"
#include <iostream>
#include "../gr-dvbs2rx_amd/csrc/spectrum_hip.h"
#include "host_main.h"

static unsigned long long bits_of(double f) { unsigned long long b; std::memcpy(&b, &f, 8); return b; }

static void print_floats(const std::vector<float>& v)
{
    for (float f : v) std::printf("%08x ", to_bits(f));
    std::printf("\n");
}

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "geom") {
            int nfft, hop, avg, n_in, n_seg = -1, n_rows = -1, used = -1;
            is >> nfft >> hop >> avg >> n_in;
            if (dvbs2::spectrum_geometry(nfft, hop, avg, n_in, &n_seg, &n_rows, &used)) std::printf("refused\n");
            else std::printf("%d %d %d\n", n_seg, n_rows, used);
        } else if (what == "window") {
            int kind, nfft;
            is >> kind >> nfft;
            std::vector<float> w((size_t)(nfft > 0 && nfft <= 8192 ? nfft : 1));
            if (dvbs2::spectrum_window(kind, nfft, w.data())) std::printf("refused\n");
            else print_floats(w);
        } else if (what == "twiddles") {
            int nfft;
            is >> nfft;
            std::vector<float> t((size_t)(nfft > 0 && nfft <= 8192 ? nfft : 1)); // nfft / 2 pairs
            if (dvbs2::spectrum_twiddles(nfft, t.data())) std::printf("refused\n");
            else print_floats(t);
        } else if (what == "check") {
            int nfft, hop, avg, max_streams, max_samples, n;
            is >> nfft >> hop >> avg >> max_streams >> max_samples >> n;
            const std::vector<float> w = read_taps(is, n);
            const std::string bad = dvbs2::SpectrumHip::check_args(nfft, hop, avg, w.empty() ? nullptr : w.data(), max_streams, max_samples);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else if (what == "carriers") {
            int shifted, nfft;
            dvbs2::SpectrumCarrierParams p = dvbs2::kSpectrumCarrierDefaults;
            is >> shifted >> p.smooth >> p.floor_quantile >> p.threshold_db >> p.min_gap >> p.min_width >> nfft;
            const std::vector<float> row = read_taps(is, nfft > 0 ? nfft : 0);
            const std::string bad = dvbs2::spectrum_carriers_check(row.empty() ? nullptr : row.data(), nfft, p);
            if (!bad.empty()) { std::printf("refused: %s\n", bad.c_str()); continue; }
            const std::vector<dvbs2::SpectrumCarrier> found = dvbs2::spectrum_carriers(row.data(), nfft, shifted != 0, p);
            std::printf("%d", (int)found.size());
            for (const auto& c : found)
                std::printf(" %016llx %016llx %016llx %016llx %d %d", bits_of(c.centre), bits_of(c.bandwidth), bits_of(c.level), bits_of(c.floor),
                            c.lo_bin, c.hi_bin);
            std::printf("\n");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
