// stdin rows -> one line each. Drives the host side of the rotator rows' C ABI (dvbs2_rotator_state_init, _state_read, _adjust_turns,
// _rows_check, and the argument checks of the three _device entries) outside Python, so that it can be built with
// -fsanitize=address,undefined together with the sources behind the entries (csrc/c_api_rotator_rows.hip and csrc/rotator_rows_hip.hip).
// No device code runs and no GPU call is made: every row is answered before a device is looked for, and a row whose arguments pass every
// check comes back as "-2: this program looks for no device". Doubles travel as the hexadecimal bits of a float64, floats as those of a
// float32, 64-bit integers in decimal (unsigned ones in hexadecimal), addresses in hexadecimal: they are never dereferenced.
//   init n d0 .. d(n-1)     -> "ok inc0 .. inc(n-1)" (hex) or "refused -1: <text>" followed by " untouched" / " WRITTEN"
//   read phase inc          -> "ok <bits of phase_inc> <bits of phase_at_index>"
//   adjust e scale          -> "ok <delta> <applies>"
//   check in_stride out_stride n_samples n_streams base_index
//   rows in in_stride out out_stride n_samples n_streams base_index state
//   retune state stream_index at_index phase_inc
//   control offsets n_streams max_slots cf cc ne ff fv coarse_scale fine_scale at_index state applied delta
//   null                    -> the null-pointer refusals of the host entries
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"

static double read_double(std::istringstream& is)
{
    uint64_t b = 0;
    is >> std::hex >> b >> std::dec;
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}
static uint64_t double_bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static uint64_t read_hex(std::istringstream& is) { uint64_t b = 0; is >> std::hex >> b >> std::dec; return b; }
template <class T> static T* addr(std::istringstream& is) { return reinterpret_cast<T*>((uintptr_t)read_hex(is)); }

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        dvbs2::g_api_error = "stale";
        if (what == "init") {
            int n;
            is >> n;
            std::vector<double> inc;
            for (int i = 0; i < n; i++) inc.push_back(read_double(is));
            const dvbs2_rotator_state_t fill = { 0x1111111111111111ull, 0x2222222222222222ull, 0x3333333333333333ll, 0x4444444444444444ull };
            std::vector<dvbs2_rotator_state_t> st((size_t)(n > 0 ? n : 0), fill); // exactly n records: one more is the sanitizer's to find
            const int code = dvbs2_rotator_state_init(inc.data(), n, st.data());
            if (code) {
                bool same = true;
                for (const auto& r : st) same = same && std::memcmp(&r, &fill, sizeof r) == 0;
                std::printf("refused %d: %s %s\n", code, dvbs2::g_api_error.c_str(), same ? "untouched" : "WRITTEN");
            } else {
                std::printf("ok");
                for (const auto& r : st) {
                    if (r.phase != 0 || r.index != 0 || r.reserved != 0) { std::printf(" bad record\n"); return 1; }
                    std::printf(" %llx", (unsigned long long)r.inc);
                }
                std::printf("\n");
            }
        } else if (what == "read") {
            dvbs2_rotator_state_t st = { read_hex(is), 0, 5, 9 };
            st.inc = read_hex(is);
            double inc = 0, phase = 0;
            const int code = dvbs2_rotator_state_read(&st, 1, &inc, &phase);
            if (code || dvbs2_rotator_state_read(&st, 1, nullptr, nullptr)) answer("", code ? code : -9);
            else std::printf("ok %llx %llx\n", (unsigned long long)double_bits(inc), (unsigned long long)double_bits(phase));
        } else if (what == "adjust") {
            const float e = read_float(is);
            const double scale = read_double(is);
            int64_t delta = 7;
            int applies = 7;
            const int code = dvbs2_rotator_adjust_turns(e, scale, &delta, &applies);
            if (code) answer("", code);
            else std::printf("ok %lld %d\n", (long long)delta, applies);
        } else if (what == "check") {
            int64_t in_stride, out_stride, base;
            int n, S;
            is >> in_stride >> out_stride >> n >> S >> base;
            answer("", dvbs2_rotator_rows_check(in_stride, out_stride, n, S, base));
        } else if (what == "rows") {
            const float* in = addr<float>(is);
            int64_t in_stride, out_stride, base;
            int n, S;
            is >> in_stride;
            float* out = addr<float>(is);
            is >> out_stride >> n >> S >> base;
            const dvbs2_rotator_state_t* st = addr<dvbs2_rotator_state_t>(is);
            answer("", dvbs2_rotator_rows_device(in, in_stride, out, out_stride, n, S, base, st, 0, nullptr));
        } else if (what == "retune") {
            dvbs2_rotator_state_t* st = addr<dvbs2_rotator_state_t>(is);
            int idx;
            int64_t at;
            is >> idx >> at;
            const double inc = read_double(is);
            answer("", dvbs2_rotator_retune_device(st, idx, at, inc, 0, nullptr));
        } else if (what == "control") {
            const int32_t* off = addr<int32_t>(is);
            int S, max_slots;
            is >> S >> max_slots;
            const float* cf = addr<float>(is);
            const int32_t* cc = addr<int32_t>(is);
            const int32_t* ne = addr<int32_t>(is);
            const float* ff = addr<float>(is);
            const int32_t* fv = addr<int32_t>(is);
            const double cs = read_double(is), fs = read_double(is);
            int64_t at;
            is >> at;
            dvbs2_rotator_state_t* st = addr<dvbs2_rotator_state_t>(is);
            int32_t* applied = addr<int32_t>(is);
            int64_t* delta = addr<int64_t>(is);
            answer("", dvbs2_rotator_control_device(off, S, max_slots, cf, cc, ne, ff, fv, cs, fs, at, st, applied, delta, 0, nullptr));
        } else if (what == "null") {
            double d[1] = { 0.25 };
            dvbs2_rotator_state_t st[1] = {};
            int64_t delta = 7;
            int applies = 7;
            answer("init-inc", dvbs2_rotator_state_init(nullptr, 1, st));
            answer("init-state", dvbs2_rotator_state_init(d, 1, nullptr));
            answer("init-count", dvbs2_rotator_state_init(d, 0, st));
            answer("read-state", dvbs2_rotator_state_read(nullptr, 1, d, d));
            answer("read-count", dvbs2_rotator_state_read(st, 65536, d, d));
            answer("adjust-delta", dvbs2_rotator_adjust_turns(0.0f, 1.0, nullptr, &applies));
            answer("adjust-applies", dvbs2_rotator_adjust_turns(0.0f, 1.0, &delta, nullptr));
            std::printf("outputs %s\n", delta == 7 && applies == 7 && d[0] == 0.25 ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
