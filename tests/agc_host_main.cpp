// stdin rows -> one line each. Drives the host-only side of the AGC's C ABI (dvbs2_agc_check, and every dvbs2_agc_* entry with a null
// handle) outside Python, so that it can be built with -fsanitize=address,undefined together with the sources behind the entries
// (csrc/c_api_agc.hip and csrc/agc_hip.hip, which it binds). No device code runs and no GPU call is made: every row is answered before a
// device is looked for. Floats travel as the hexadecimal bits of a float32, so they arrive exactly.
//   check rate reference gain max_gain                      -> "ok" or "refused -1: <text>"
//   create rate reference gain max_gain max_streams max_samples -> "refused <code>: <text>" (only refused rows are sent)
//   null                                                    -> one "<entry> <code>: <text>" line per entry called with a null handle
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
            const float rate = read_float(is), reference = read_float(is), gain = read_float(is), max_gain = read_float(is);
            dvbs2::g_api_error = "stale";
            answer("", dvbs2_agc_check(rate, reference, gain, max_gain));
        } else if (what == "create") {
            const float rate = read_float(is), reference = read_float(is), gain = read_float(is), max_gain = read_float(is);
            int max_streams, max_samples;
            is >> max_streams >> max_samples;
            dvbs2_agc_t* h = reinterpret_cast<dvbs2_agc_t*>(1); // must come back null
            const int code = dvbs2_agc_create(&h, rate, reference, gain, max_gain, max_streams, max_samples, 0);
            if (h) { std::printf("handle not cleared\n"); return 1; }
            answer("", code);
        } else if (what == "null") {
            float f[3] = { 7.0f, 7.0f, 7.0f }, buf[4] = {};
            int v[2] = { 7, 7 };
            answer("reset", dvbs2_agc_reset(nullptr));
            answer("set_params", dvbs2_agc_set_params(nullptr, 1e-5f, 1.0f, 65536.0f));
            answer("set_swap_iq", dvbs2_agc_set_swap_iq(nullptr, 1));
            answer("set_gain", dvbs2_agc_set_gain(nullptr, -1, 1.0f));
            answer("params", dvbs2_agc_params(nullptr, &f[0], &f[1], &f[2], &v[0], &v[1]));
            answer("state", dvbs2_agc_state(nullptr, buf, 4));
            answer("work_device", dvbs2_agc_work_device(nullptr, buf, 2, 2, 1, buf, 2, buf, 2, nullptr));
            answer("work", dvbs2_agc_work(nullptr, buf, 2, buf, buf));
            answer("create", dvbs2_agc_create(nullptr, 1e-5f, 1.0f, 1.0f, 65536.0f, 1, 16, 0));
            dvbs2_agc_destroy(nullptr);
            std::printf("destroy %s\n", f[0] == 7.0f && f[1] == 7.0f && f[2] == 7.0f && v[0] == 7 && v[1] == 7 ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
