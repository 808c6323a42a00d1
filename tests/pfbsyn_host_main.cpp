// stdin rows -> one line each. Drives the host-only side of the polyphase synthesizer (csrc/pfbsyn_hip.hip: geometry, the tile rule, the
// counter, the argument checks of the class; csrc/c_api_pfbsyn.hip: dvbs2_pfbsyn_check, dvbs2_pfbsyn_tile, the refusals of
// dvbs2_pfbsyn_create and every dvbs2_pfbsyn_* entry with a null handle) outside Python, so that it can be built with
// -fsanitize=address,undefined. No device code runs and no GPU call is made: every row is answered before a device is looked for.
// Floats travel as the hexadecimal bits of a float32, so both directions are exact.
//   geom n_chan interp ntaps                      -> "tail delay_num taps_per_phase" or "refused"
//   tile n_chan interp ntaps                      -> "tile" (the class's rule and the entry's, which must agree) or "refused -1: <text>"
//   seq position k n_in ... n_in                  -> the counter behind every call; "refused" ends the row
//   check n_chan interp max_streams max_samples n tap ... tap -> "ok" or "refused -1: <text>" (dvbs2_pfbsyn_check)
//   create n_chan interp max_streams max_samples n tap ... tap -> "refused <code>: <text>" (only refused rows are sent)
//   channels n_chan n c ... c                     -> "ok" or "refused: <text>" (PfbsynHip::check_channels)
//   null                                          -> one "<entry> <code>: <text>" line per entry called with a null handle
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"
#include "../gr-dvbs2rx_amd/csrc/pfbsyn_hip.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "geom") {
            int n_chan, interp, ntaps, tail = -1, delay = -1, per_phase = -1;
            is >> n_chan >> interp >> ntaps;
            if (dvbs2::pfbsyn_geometry(n_chan, interp, ntaps, &tail, &delay, &per_phase)) std::printf("refused\n");
            else std::printf("%d %d %d\n", tail, delay, per_phase);
        } else if (what == "tile") {
            int n_chan, interp, ntaps;
            is >> n_chan >> interp >> ntaps;
            const int tile = dvbs2_pfbsyn_tile(n_chan, interp, ntaps);
            if (tile < 0) { answer("", tile); continue; }
            if (tile != dvbs2::pfbsyn_tile(n_chan, interp, ntaps)) { std::printf("the class disagrees\n"); return 1; }
            std::printf("%d\n", tile);
        } else if (what == "seq") {
            long long counter;
            int k;
            is >> counter >> k;
            for (int i = 0; i < k; i++) {
                int n_in;
                is >> n_in;
                const int64_t next = dvbs2::pfbsyn_advance(counter, n_in);
                if (next < 0) { std::printf("refused "); break; }
                counter = next;
                std::printf("%lld ", counter);
            }
            std::printf("\n");
        } else if (what == "check" || what == "create") {
            int n_chan, interp, max_streams, max_samples, n;
            is >> n_chan >> interp >> max_streams >> max_samples >> n;
            const std::vector<float> t = read_taps(is, n);
            const float* taps = t.empty() ? nullptr : t.data();
            dvbs2::g_api_error = "stale";
            if (what == "check") {
                answer("", dvbs2_pfbsyn_check(n_chan, interp, taps, n, max_streams, max_samples));
                const std::string bad = dvbs2::PfbsynHip::check_args(n_chan, interp, taps, n, max_streams, max_samples);
                if (bad.empty() != (dvbs2::g_api_error == "stale") || (!bad.empty() && bad != dvbs2::g_api_error)) { std::printf("the class disagrees\n"); return 1; }
            } else {
                dvbs2_pfbsyn_t* h = reinterpret_cast<dvbs2_pfbsyn_t*>(1); // must come back null
                const int code = dvbs2_pfbsyn_create(&h, n_chan, interp, taps, n, max_streams, max_samples, 0);
                if (h) { std::printf("handle not cleared\n"); return 1; }
                answer("", code);
            }
        } else if (what == "channels") {
            int n_chan, n;
            is >> n_chan >> n;
            std::vector<int> list; // exactly n values (n < 0: a null list said to hold -n)
            for (int i = 0; i < n; i++) { int c; is >> c; list.push_back(c); }
            const std::string bad = dvbs2::PfbsynHip::check_channels(n_chan, list.empty() ? nullptr : list.data(), n < 0 ? -n : n);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else if (what == "null") {
            float buf[4] = {};
            int v[6] = { 7, 7, 7, 7, 7, 7 }, list[2] = { 0, 1 };
            int64_t n = 7;
            answer("reset", dvbs2_pfbsyn_reset(nullptr));
            answer("set_channels", dvbs2_pfbsyn_set_channels(nullptr, list, 2));
            answer("params", dvbs2_pfbsyn_params(nullptr, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]));
            answer("position", dvbs2_pfbsyn_position(nullptr, &n));
            answer("channels", dvbs2_pfbsyn_channels(nullptr, list, &v[0]));
            answer("process_device", dvbs2_pfbsyn_process_device(nullptr, buf, 2, 2, 1, buf, 2, &n, nullptr));
            answer("process", dvbs2_pfbsyn_process(nullptr, buf, 2, 2, 1, buf, 2, &n));
            answer("create", dvbs2_pfbsyn_create(nullptr, 8, 4, buf, 4, 1, 16, 0));
            dvbs2_pfbsyn_destroy(nullptr);
            bool clean = n == 7 && list[0] == 0 && list[1] == 1;
            for (int x : v) clean = clean && x == 7;
            std::printf("destroy %s\n", clean ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
