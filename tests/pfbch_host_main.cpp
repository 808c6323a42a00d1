// stdin rows -> one line each. Drives the host-only side of the polyphase channelizer (csrc/pfbch_hip.hip: geometry, the count rule, the
// tile rule, the twiddle table, the argument checks of the class; csrc/c_api_pfbch.hip: dvbs2_pfbch_check, the refusals of
// dvbs2_pfbch_create and every dvbs2_pfbch_* entry with a null handle) outside Python, so that it can be built with
// -fsanitize=address,undefined. No device code runs and no GPU call is made: every row is answered before a device is looked for.
// Floats travel as the hexadecimal bits of a float32, so both directions are exact.
//   geom n_chan decim ntaps                       -> "history delay_num taps_per_branch" or "refused"
//   produce position decim n_in                   -> "n" or "refused"
//   seq position decim k n_in ... n_in            -> "n_out counter" per call, the counter carried over; "refused" ends the row
//   tile n_chan decim ntaps                       -> "tile"
//   tw n_chan                                     -> the n_chan / 2 pairs as hexadecimal bits, or "refused"
//   check n_chan decim max_streams max_samples n tap ... tap -> "ok" or "refused -1: <text>" (dvbs2_pfbch_check)
//   create n_chan decim max_streams max_samples n tap ... tap -> "refused <code>: <text>" (only refused rows are sent)
//   channels n_chan n c ... c                     -> "ok" or "refused: <text>" (PfbchHip::check_channels)
//   null                                          -> one "<entry> <code>: <text>" line per entry called with a null handle
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"
#include "../gr-dvbs2rx_amd/csrc/pfbch_hip.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "geom") {
            int n_chan, decim, ntaps, history = -1, delay = -1, per_branch = -1;
            is >> n_chan >> decim >> ntaps;
            if (dvbs2::pfbch_geometry(n_chan, decim, ntaps, &history, &delay, &per_branch)) std::printf("refused\n");
            else std::printf("%d %d %d\n", history, delay, per_branch);
        } else if (what == "produce") {
            long long position;
            int decim, n_in;
            is >> position >> decim >> n_in;
            const int64_t n = dvbs2::pfbch_produce(position, decim, n_in);
            if (n < 0) std::printf("refused\n");
            else std::printf("%lld\n", (long long)n);
        } else if (what == "seq") {
            long long counter;
            int decim, k;
            is >> counter >> decim >> k;
            for (int i = 0; i < k; i++) {
                int n_in;
                is >> n_in;
                const int64_t n = dvbs2::pfbch_produce(counter, decim, n_in);
                if (n < 0) { std::printf("refused "); break; }
                counter += n_in;
                std::printf("%lld %lld ", (long long)n, counter);
            }
            std::printf("\n");
        } else if (what == "tile") {
            int n_chan, decim, ntaps;
            is >> n_chan >> decim >> ntaps;
            std::printf("%d\n", dvbs2::pfbch_tile(n_chan, decim, ntaps));
        } else if (what == "tw") {
            int n_chan;
            is >> n_chan;
            std::vector<float> t(n_chan > 1 && n_chan <= 256 ? (size_t)(n_chan / 2) * 2 : 0); // exactly the pairs the entry writes
            if (dvbs2_pfbch_twiddles(n_chan, t.empty() ? nullptr : t.data())) { std::printf("refused\n"); continue; }
            for (float f : t) std::printf("%08x ", to_bits(f));
            std::printf("\n");
        } else if (what == "check" || what == "create") {
            int n_chan, decim, max_streams, max_samples, n;
            is >> n_chan >> decim >> max_streams >> max_samples >> n;
            const std::vector<float> t = read_taps(is, n);
            const float* taps = t.empty() ? nullptr : t.data();
            dvbs2::g_api_error = "stale";
            if (what == "check") {
                answer("", dvbs2_pfbch_check(n_chan, decim, taps, n, max_streams, max_samples));
                const std::string bad = dvbs2::PfbchHip::check_args(n_chan, decim, taps, n, max_streams, max_samples);
                if (bad.empty() != (dvbs2::g_api_error == "stale") || (!bad.empty() && bad != dvbs2::g_api_error)) { std::printf("the class disagrees\n"); return 1; }
            } else {
                dvbs2_pfbch_t* h = reinterpret_cast<dvbs2_pfbch_t*>(1); // must come back null
                const int code = dvbs2_pfbch_create(&h, n_chan, decim, taps, n, max_streams, max_samples, 0);
                if (h) { std::printf("handle not cleared\n"); return 1; }
                answer("", code);
            }
        } else if (what == "channels") {
            int n_chan, n;
            is >> n_chan >> n;
            std::vector<int> list; // exactly n values (n < 0: a null list said to hold -n)
            for (int i = 0; i < n; i++) { int c; is >> c; list.push_back(c); }
            const std::string bad = dvbs2::PfbchHip::check_channels(n_chan, list.empty() ? nullptr : list.data(), n < 0 ? -n : n);
            std::printf("%s%s\n", bad.empty() ? "ok" : "refused: ", bad.c_str());
        } else if (what == "null") {
            float buf[4] = {};
            int v[6] = { 7, 7, 7, 7, 7, 7 }, list[2] = { 0, 1 };
            int64_t n = 7;
            answer("reset", dvbs2_pfbch_reset(nullptr));
            answer("set_channels", dvbs2_pfbch_set_channels(nullptr, list, 2));
            answer("params", dvbs2_pfbch_params(nullptr, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]));
            answer("position", dvbs2_pfbch_position(nullptr, &n));
            answer("channels", dvbs2_pfbch_channels(nullptr, list, &v[0]));
            answer("process_device", dvbs2_pfbch_process_device(nullptr, buf, 2, 2, 1, buf, 2, &n, nullptr));
            answer("process", dvbs2_pfbch_process(nullptr, buf, 2, 2, 1, buf, 2, &n));
            answer("create", dvbs2_pfbch_create(nullptr, 8, 4, buf, 4, 1, 16, 0));
            dvbs2_pfbch_destroy(nullptr);
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
