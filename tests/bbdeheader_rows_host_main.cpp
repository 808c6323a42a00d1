// stdin rows -> one line each. Drives the host side of the de-header rows' C ABI (dvbs2_bbdeheader_rows_check, _rows_geometry,
// _state_counters and the argument checks of dvbs2_bbdeheader_rows_device) outside Python, so that it can be built with
// -fsanitize=address,undefined together with the sources behind the entries (csrc/c_api_bbdeheader_rows.hip and
// csrc/bbdeheader_rows_hip.hip). No device code runs and no GPU call is made: every row is answered before a device is looked for, and a
// row whose arguments pass every check comes back as "-2: this program looks for no device". Integers travel in decimal, addresses in
// hexadecimal: they are never dereferenced.
//   check kbch_bits n_streams max_frames
//   geometry kbch_bits n_streams max_frames  -> "ok kbch_bytes max_out_bytes_per_frame work_bytes out_bytes", or the refusal followed by
//                                               " untouched" / " WRITTEN"
//   counters n, then per record: synched partial packets errors bbframes dropped gaps overruns
//                                            -> "ok" and per record: packets errors bbframes dropped gaps overruns synched partial
//   rows bbframes kbch_bits offsets n_streams max_frames state work work_bytes ts_out out_bytes pkt_offsets
//   null                                     -> the null-pointer and count refusals of dvbs2_bbdeheader_state_counters
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"

static uint64_t read_hex(std::istringstream& is) { uint64_t b = 0; is >> std::hex >> b >> std::dec; return b; }
template <class T> static T* addr(std::istringstream& is) { return reinterpret_cast<T*>((uintptr_t)read_hex(is)); }

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        dvbs2::g_api_error = "stale";
        if (what == "check") {
            int kbch, S, mf;
            is >> kbch >> S >> mf;
            answer("", dvbs2_bbdeheader_rows_check(kbch, S, mf));
        } else if (what == "geometry") {
            int kbch, S, mf;
            is >> kbch >> S >> mf;
            int kb = -7, mo = -7;
            int64_t wb = -7, ob = -7;
            const int code = dvbs2_bbdeheader_rows_geometry(kbch, S, mf, &kb, &mo, &wb, &ob);
            if (code) {
                std::printf("refused %d: %s %s\n", code, dvbs2::g_api_error.c_str(), kb == -7 && mo == -7 && wb == -7 && ob == -7 ? "untouched" : "WRITTEN");
            } else if (dvbs2_bbdeheader_rows_geometry(kbch, S, mf, nullptr, nullptr, nullptr, nullptr)) { // every output is nullable
                answer("", -9);
            } else {
                std::printf("ok %d %d %lld %lld\n", kb, mo, (long long)wb, (long long)ob);
            }
        } else if (what == "counters") {
            int n;
            is >> n;
            std::vector<dvbs2_bbdeheader_state_t> st((size_t)(n > 0 ? n : 0)); // exactly n records: one more is the sanitizer's to find
            for (auto& r : st) {
                std::memset(&r, 0xEE, sizeof r);
                is >> r.synched >> r.partial_ts_bytes >> r.packets >> r.errors >> r.bbframes >> r.dropped >> r.gaps >> r.overruns;
            }
            std::vector<dvbs2_bbdeheader_counters_t> out(st.size());
            const int code = dvbs2_bbdeheader_state_counters(st.data(), n, out.data());
            if (code) { answer("", code); continue; }
            std::printf("ok");
            for (const auto& c : out)
                std::printf(" %llu %llu %llu %llu %llu %llu %d %d", (unsigned long long)c.packets, (unsigned long long)c.errors, (unsigned long long)c.bbframes,
                            (unsigned long long)c.dropped, (unsigned long long)c.gaps, (unsigned long long)c.overruns, c.synched, c.partial_ts_bytes);
            std::printf("\n");
        } else if (what == "rows") {
            const uint8_t* bb = addr<uint8_t>(is);
            int kbch, S, mf;
            int64_t work_bytes, out_bytes;
            is >> kbch;
            const int32_t* off = addr<int32_t>(is);
            is >> S >> mf;
            dvbs2_bbdeheader_state_t* st = addr<dvbs2_bbdeheader_state_t>(is);
            void* work = addr<void>(is);
            is >> work_bytes;
            uint8_t* out = addr<uint8_t>(is);
            is >> out_bytes;
            int32_t* pko = addr<int32_t>(is);
            answer("", dvbs2_bbdeheader_rows_device(bb, kbch, off, S, mf, st, work, work_bytes, out, out_bytes, pko, 0, nullptr));
        } else if (what == "null") {
            dvbs2_bbdeheader_state_t st[1] = {};
            dvbs2_bbdeheader_counters_t out[1];
            std::memset(out, 0x77, sizeof out);
            dvbs2_bbdeheader_counters_t same[1];
            std::memcpy(same, out, sizeof out);
            answer("counters-state", dvbs2_bbdeheader_state_counters(nullptr, 1, out));
            answer("counters-out", dvbs2_bbdeheader_state_counters(st, 1, nullptr));
            answer("counters-none", dvbs2_bbdeheader_state_counters(st, 0, out));
            answer("counters-many", dvbs2_bbdeheader_state_counters(st, 1025, out));
            std::printf("outputs %s\n", std::memcmp(same, out, sizeof out) == 0 ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
