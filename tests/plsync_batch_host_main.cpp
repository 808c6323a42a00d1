// stdin rows -> one line each. Drives the host-only side of the batched PL stages (csrc/c_api_plsync_batch.hip, csrc/plsync_batch_hip.hip:
// dvbs2_plsync_batch_check, dvbs2_plsync_batch_check_search and the refusals of dvbs2_plsync_batch_create; csrc/c_api_plcoarse.hip: the
// refusals of dvbs2_plcoarse_batch_create; csrc/c_api_plframe.hip: dvbs2_plframe_stride_check; every entry of
// the batched stages of include/dvbs2_fec_hip.h with a null handle) outside Python, so that it can be built with -fsanitize=address,undefined. No device
// code runs and no GPU call is made: every row is answered before a device is looked for.
//   check plsc unlock_thresh max_streams max_symbols max_frames   -> "ok" or "refused <code>: <text>" (dvbs2_plsync_batch_check; the class's
//                                                                    rule must agree)
//   create plsc unlock_thresh max_streams max_symbols max_frames  -> "refused <code>: <text>" (dvbs2_plsync_batch_create)
//   coarse period plsc max_streams max_slots                      -> "refused <code>: <text>" (dvbs2_plcoarse_batch_create)
//   search max_streams max_symbols stride n_streams has_first has_n_syms first ... n_syms ...  (n_streams values each, exactly)
//                                                                 -> "ok" or "refused <code>: <text>" (dvbs2_plsync_batch_check_search)
//   stride plsc stride_syms                                       -> "ok" or "refused <code>: <text>" (dvbs2_plframe_stride_check)
//   null                                                          -> one "<entry> <code>: <text>" line per entry called with a null handle
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"
#include "../gr-dvbs2rx_amd/csrc/plcoarse_hip.h"
#include "../gr-dvbs2rx_amd/csrc/plsync_batch_hip.h"

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "check" || what == "create") {
            int plsc, ut, ms, mn, mf;
            is >> plsc >> ut >> ms >> mn >> mf;
            dvbs2::g_api_error = "stale";
            if (what == "check") {
                answer("", dvbs2_plsync_batch_check(plsc, ut, ms, mn, mf));
                const std::string bad = dvbs2::plsync_batch_check(plsc, ut, ms, mn, mf);
                if (bad.empty() != (dvbs2::g_api_error == "stale") || (!bad.empty() && bad != dvbs2::g_api_error)) { std::printf("the class disagrees\n"); return 1; }
            } else {
                dvbs2_plsync_batch_t* h = reinterpret_cast<dvbs2_plsync_batch_t*>(1); // must come back null
                const int code = dvbs2_plsync_batch_create(&h, plsc, ut, ms, mn, mf, 0);
                if (h) { std::printf("handle not cleared\n"); return 1; }
                answer("", code);
            }
        } else if (what == "coarse") {
            int period, plsc, ms, slots;
            is >> period >> plsc >> ms >> slots;
            dvbs2_plcoarse_batch_t* h = reinterpret_cast<dvbs2_plcoarse_batch_t*>(1);
            const int code = dvbs2_plcoarse_batch_create(&h, period, plsc, ms, slots, 0);
            if (h) { std::printf("handle not cleared\n"); return 1; }
            answer("", code);
            const std::string bad = dvbs2::plcoarse_batch_check(period, plsc, ms, slots);
            if (bad.empty() != (code == DVBS2_EDEVICE) || (!bad.empty() && bad != dvbs2::g_api_error)) { std::printf("the class disagrees\n"); return 1; }
        } else if (what == "search") {
            int ms, mn, n, has_first, has_n;
            long long stride;
            is >> ms >> mn >> stride >> n >> has_first >> has_n;
            std::vector<int> first, count; // exactly n values each: a read past the end is the sanitizer's to find
            for (int i = 0; i < n; i++) { int v; is >> v; first.push_back(v); }
            for (int i = 0; i < n; i++) { int v; is >> v; count.push_back(v); }
            answer("", dvbs2_plsync_batch_check_search(ms, mn, stride, has_first ? first.data() : nullptr, has_n ? count.data() : nullptr, n));
        } else if (what == "stride") {
            int plsc;
            long long stride;
            is >> plsc >> stride;
            answer("", dvbs2_plframe_stride_check(plsc, stride));
        } else if (what == "null") {
            float buf[4] = {};
            int v[3] = { 7, 7, 7 }, two[2] = { 0, 1 };
            int32_t w[3] = { 7, 7, 7 };
            uint8_t list[2] = { 0, 1 };
            dvbs2_plsync_frame_t rec = {};
            answer("batch_reset", dvbs2_plsync_batch_reset(nullptr));
            answer("batch_reset_stream", dvbs2_plsync_batch_reset_stream(nullptr, 0));
            answer("batch_set_plsc_mode", dvbs2_plsync_batch_set_plsc_mode(nullptr, 1, 1));
            answer("batch_set_expected_pls", dvbs2_plsync_batch_set_expected_pls(nullptr, list, 2));
            answer("batch_search_device", dvbs2_plsync_batch_search_device(nullptr, buf, 2, two, two, 2, &rec, nullptr));
            answer("batch_finish", dvbs2_plsync_batch_finish(nullptr, &v[0], &v[1], &v[2]));
            answer("batch_gather_device", dvbs2_plsync_batch_gather_device(nullptr, buf, 2, &rec, 1, 7, buf, 1, w, w, nullptr));
            answer("estimate_strided_device", dvbs2_plframe_estimate_strided_device(nullptr, buf, 9000, 1, w, buf, nullptr, nullptr));
            answer("process_strided_device", dvbs2_plframe_process_strided_device(nullptr, buf, 9000, 1, w, buf, buf, nullptr, nullptr));
            answer("coarse_batch_reset", dvbs2_plcoarse_batch_reset(nullptr));
            answer("coarse_batch_reset_stream", dvbs2_plcoarse_batch_reset_stream(nullptr, 0));
            answer("coarse_batch_estimate_device", dvbs2_plcoarse_batch_estimate_device(nullptr, buf, 90, list, w, 1, buf, w, w, nullptr));
            answer("batch_create", dvbs2_plsync_batch_create(nullptr, -1, 3, 1, 40000, 16, 0));
            answer("coarse_batch_create", dvbs2_plcoarse_batch_create(nullptr, 1, -1, 1, 16, 0));
            dvbs2_plsync_batch_destroy(nullptr);
            dvbs2_plcoarse_batch_destroy(nullptr);
            bool clean = two[0] == 0 && two[1] == 1 && rec.sof_index == 0;
            for (int x : v) clean = clean && x == 7;
            for (int32_t x : w) clean = clean && x == 7;
            std::printf("destroy %s\n", clean ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
