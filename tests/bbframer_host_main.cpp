// stdin rows -> one line each. Drives the host-only code of the BB framer (csrc/bbframer_hip.hip: BBHEADER, CRC-8, the packet arithmetic
// of a call, the argument checks) outside Python, so that it can be built with -fsanitize=address,undefined. No device code runs.
//   hdr matype1 matype2 upl_bits dfl_bits sync syncd_bits -> the ten bytes in hex, or "refused"
//   crc n hex                                             -> the check byte (n bytes; "-" for none)
//   need pos n_frames dfl_bytes                           -> packets the call reads
//   create kbch_bits max_frames                           -> "ok" or "refused: <text>"
//   call max_frames max_dfl_bytes n_frames dfl_bytes      -> "ok" or "refused <code>: <text>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <vector>
#include "../gr-dvbs2rx_amd/csrc/bbframer_hip.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "hdr") {
            int m1, m2, upl, dfl, sync, syncd;
            is >> m1 >> m2 >> upl >> dfl >> sync >> syncd;
            std::vector<uint8_t> h(10); // exactly ten bytes: a write past the end is the sanitizer's to find
            if (dvbs2::bbheader_build(h.data(), m1, m2, upl, dfl, sync, syncd)) { std::printf("refused\n"); continue; }
            for (uint8_t b : h) std::printf("%02x", b);
            std::printf("\n");
        } else if (what == "crc") {
            size_t n;
            std::string hex;
            is >> n >> hex;
            std::vector<uint8_t> d; // exactly n bytes
            for (size_t i = 0; i < n; i++) d.push_back((uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16));
            std::printf("%d\n", dvbs2::crc8(d.empty() ? nullptr : d.data(), n));
        } else if (what == "need") {
            unsigned long long pos;
            int n_frames, dfl;
            is >> pos >> n_frames >> dfl;
            std::printf("%lld\n", (long long)dvbs2::bbframer_need(pos, n_frames, dfl));
        } else if (what == "create") {
            int kbch_bits, max_frames;
            is >> kbch_bits >> max_frames;
            const std::string bad = dvbs2::bbframer_check_create(kbch_bits, max_frames);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else if (what == "call") {
            int max_frames, max_dfl, n_frames, dfl;
            is >> max_frames >> max_dfl >> n_frames >> dfl;
            std::string text;
            const int code = dvbs2::bbframer_check_call(max_frames, max_dfl, n_frames, dfl, &text);
            if (code) std::printf("refused %d: %s\n", code, text.c_str());
            else std::printf("ok\n");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
