// stdin rows -> one line each. Drives the host-only side of the IQ sample converter's C ABI (dvbs2_iqconv_bytes, dvbs2_iqconv_check, the
// argument checks of create, the host restatement dvbs2_iqconv_unpack_host / dvbs2_iqconv_pack_host, and every dvbs2_iqconv_* entry with
// a null handle) outside Python, so that it can be built with -fsanitize=address,undefined together with the sources behind the entries
// (csrc/c_api_iqconv.hip, csrc/iqconv_hip.hip). No device code runs and no GPU call is made: every row is answered before a device is
// looked for. Floats travel as the hexadecimal bits of a float32, so they arrive exactly.
//   bytes format                                   -> the answer
//   check format gain max_streams max_samples      -> "ok" or "refused -1: <text>"
//   create format gain max_streams max_samples     -> "refused <code>: <text>" (only refused rows are sent)
//   unpack format gain offset n <2n codes>         -> "<2n float bits> | samples clipped energy"; the codes lie `offset` bytes into a
//   pack format gain offset n <2n float bits>      -> "<2n codes> | samples clipped energy"        malloc'ed buffer of exactly the
//                                                     row's size behind the offset, and so does the other buffer of the call
//   null                                           -> one "<entry> <code>: <text>" line per entry called with a null handle
#include <cstdlib>
#include <iostream>
#define HOST_MAIN_LINKS_C_API
#include "host_main.h"

static void put_code(int format, uint8_t* p, int j, int c)
{
    if (format == DVBS2_IQ_S16) { const int16_t v = (int16_t)c; std::memcpy(p + 2 * j, &v, 2); }
    else p[j] = (uint8_t)c;
}

static int get_code(int format, const uint8_t* p, int j)
{
    if (format == DVBS2_IQ_U8) return p[j];
    if (format == DVBS2_IQ_S8) return (int8_t)p[j];
    int16_t v;
    std::memcpy(&v, p + 2 * j, 2);
    return v;
}

int main()
{
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream is(line);
        std::string what;
        is >> what;
        if (what == "bytes") {
            int format;
            is >> format;
            std::printf("%d\n", dvbs2_iqconv_bytes(format));
        } else if (what == "check" || what == "create") {
            int format, max_streams, max_samples;
            is >> format;
            const float gain = read_float(is);
            is >> max_streams >> max_samples;
            dvbs2::g_api_error = "stale";
            if (what == "check") answer("", dvbs2_iqconv_check(format, gain, max_streams, max_samples));
            else {
                dvbs2_iqconv_t* h = reinterpret_cast<dvbs2_iqconv_t*>(1); // must come back null
                const int code = dvbs2_iqconv_create(&h, format, gain, max_streams, max_samples, 0);
                if (h) { std::printf("handle not cleared\n"); return 1; }
                answer("", code);
            }
        } else if (what == "unpack" || what == "pack") {
            int format, offset, n;
            is >> format;
            const float gain = read_float(is);
            is >> offset >> n;
            const int width = dvbs2_iqconv_bytes(format) / 2;
            // sized exactly: an access outside the row is a report of AddressSanitizer
            uint8_t* codes = static_cast<uint8_t*>(std::malloc(offset + (size_t)2 * n * width));
            float* floats = static_cast<float*>(std::malloc((size_t)2 * n * 4));
            uint64_t stats[3] = { 0, 0, 0 };
            if (what == "unpack") {
                for (int j = 0; j < 2 * n; j++) { int c; is >> c; put_code(format, codes + offset, j, c); }
                if (dvbs2_iqconv_unpack_host(format, gain, codes + offset, n, floats, stats)) { std::printf("refused\n"); return 1; }
                for (int j = 0; j < 2 * n; j++) std::printf("%08x ", to_bits(floats[j]));
            } else {
                for (int j = 0; j < 2 * n; j++) floats[j] = read_float(is);
                if (dvbs2_iqconv_pack_host(format, gain, floats, n, codes + offset, stats)) { std::printf("refused\n"); return 1; }
                for (int j = 0; j < 2 * n; j++) std::printf("%d ", get_code(format, codes + offset, j));
            }
            std::printf("| %llu %llu %llu\n", (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2]);
            std::free(codes);
            std::free(floats);
        } else if (what == "null") {
            float f = 7.0f, buf[4] = {};
            uint8_t codes[8] = {};
            uint64_t stats[3] = { 7, 7, 7 };
            int v[4] = { 7, 7, 7, 7 };
            answer("set_gain", dvbs2_iqconv_set_gain(nullptr, 1.0f));
            answer("params", dvbs2_iqconv_params(nullptr, &v[0], &f, &v[1], &v[2], &v[3]));
            answer("unpack_device", dvbs2_iqconv_unpack_device(nullptr, codes, 2, 2, 1, buf, 2, stats, nullptr));
            answer("pack_device", dvbs2_iqconv_pack_device(nullptr, buf, 2, 2, 1, codes, 2, stats, nullptr));
            answer("unpack_to_device", dvbs2_iqconv_unpack_to_device(nullptr, codes, 2, buf, stats));
            answer("pack_from_device", dvbs2_iqconv_pack_from_device(nullptr, buf, 2, codes, stats));
            answer("create", dvbs2_iqconv_create(nullptr, DVBS2_IQ_U8, 1.0f, 1, 16, 0));
            dvbs2_iqconv_destroy(nullptr);
            const bool clean = f == 7.0f && v[0] == 7 && v[1] == 7 && v[2] == 7 && v[3] == 7 && stats[0] == 7 && stats[1] == 7 && stats[2] == 7;
            std::printf("destroy %s\n", clean ? "nothing written" : "an output was written");
        } else {
            std::printf("unknown row\n");
            return 1;
        }
    }
    return 0;
}
