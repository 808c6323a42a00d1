// stdin rows -> one line each. Drives the host-only side of the AWGN channel's C ABI (dvbs2_awgn_check, dvbs2_awgn_sigma, the argument
// checks of create, the host restatement dvbs2_awgn_words / dvbs2_awgn_sample, and every dvbs2_awgn_* entry with a null handle) outside
// Python, so that it can be built with -fsanitize=address,undefined together with the sources behind the entries
// (csrc/c_api_channel.hip, csrc/awgn_hip.hip). No device code runs and no GPU call is made: every row is answered before a device is
// looked for. Floats travel as the hexadecimal bits of a float32, so they arrive exactly.
//   check sigma max_streams max_samples        -> "ok" or "refused -1: <text>"
//   create sigma max_streams max_samples       -> "refused <code>: <text>" (only refused rows are sent)
//   sample seed stream_id first count          -> one "<wa> <wb> <re bits> <im bits>" line per sample (hexadecimal)
//   null                                       -> one "<entry> <code>: <text>" line per entry called with a null handle
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "check") {
            const float sigma = read_float(is);
            int max_streams, max_samples;
            is >> max_streams >> max_samples;
            dvbs2::g_api_error = "stale";
            answer("", dvbs2_awgn_check(sigma, max_streams, max_samples));
        } else if (what == "create") {
            const float sigma = read_float(is);
            int max_streams, max_samples;
            is >> max_streams >> max_samples;
            dvbs2_awgn_t* h = reinterpret_cast<dvbs2_awgn_t*>(1); // must come back null
            const int code = dvbs2_awgn_create(&h, 1, sigma, max_streams, max_samples, 0);
            if (h) { std::printf("handle not cleared\n"); return 1; }
            answer("", code);
        } else if (what == "sample") {
            unsigned long long seed, stream_id;
            long long first;
            int count;
            is >> seed >> stream_id >> first >> count;
            for (int i = 0; i < count; i++) {
                uint32_t w[2];
                float v[2];
                if (dvbs2_awgn_words(seed, stream_id, first + i, w) || dvbs2_awgn_sample(seed, stream_id, first + i, v)) { std::printf("refused\n"); return 1; }
                std::printf("%08x %08x %08x %08x\n", w[0], w[1], to_bits(v[0]), to_bits(v[1]));
            }
        } else if (what == "null") {
            float f = 7.0f, buf[4] = {};
            uint64_t seed = 7;
            int v[2] = { 7, 7 };
            answer("set_sigma", dvbs2_awgn_set_sigma(nullptr, 1.0f));
            answer("set_seed", dvbs2_awgn_set_seed(nullptr, 1));
            answer("params", dvbs2_awgn_params(nullptr, &seed, &f, &v[0], &v[1]));
            answer("add_device", dvbs2_awgn_add_device(nullptr, buf, 2, 2, 1, 0, 0, nullptr, buf, 2, nullptr));
            answer("add", dvbs2_awgn_add(nullptr, buf, 2, 0, 0, buf));
            answer("create", dvbs2_awgn_create(nullptr, 1, 1.0f, 1, 16, 0));
            dvbs2_awgn_destroy(nullptr);
            std::printf("destroy %s\n", f == 7.0f && seed == 7 && v[0] == 7 && v[1] == 7 ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
