// stdin rows "plsc plsc ..." (one sequence each, values 0..255) -> one line "in_offset:out_offset ... | in_syms out_syms" each, or
// "refused: <text>". Drives the host-only layout code of the PL framer (csrc/pl_signal.cpp) outside Python, so that it can be built
// with -fsanitize=address,undefined; it links no kernel unit.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <vector>
#include "../gr-dvbs2rx_amd/csrc/pl_signal.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::vector<uint8_t> plsc;
        for (int v; is >> v;) plsc.push_back((uint8_t)v);
        std::vector<dvbs2::PlFramerRec> rec(plsc.size()); // exactly n_frames records: a write past the end is the sanitizer's to find
        int64_t in = -1, out = -1;
        std::string why;
        if (!dvbs2::plframer_layout(plsc.data(), (int)plsc.size(), rec.data(), &in, &out, &why)) { std::printf("refused: %s\n", why.c_str()); continue; }
        for (const auto& r : rec) std::printf("%lld:%lld ", (long long)r.in_offset, (long long)r.out_offset);
        std::printf("| %lld %lld\n", (long long)in, (long long)out);
    }
    return 0;
}
