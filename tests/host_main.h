// host_main.h -- what the stand-alone host programs (tests/*_host_main.cpp, built by fec_testlib.build_host_program) share: how floats
// travel (the hexadecimal bits of a float32, so that they arrive exactly) and, for a program that links a csrc/c_api_*.hip unit and says
// so with HOST_MAIN_LINKS_C_API in front of this header, the line an entry's answer becomes and the two definitions that c_api_core.hip
// gives the library.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

inline float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
inline uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
inline float read_float(std::istringstream& is) { uint32_t b = 0; is >> std::hex >> b >> std::dec; return from_bits(b); }

inline std::vector<float> read_taps(std::istringstream& is, int n)
{
    std::vector<float> t; // exactly n floats: a read or write past the end is the sanitizer's to find
    for (int i = 0; i < n; i++) t.push_back(read_float(is));
    return t;
}

#ifdef HOST_MAIN_LINKS_C_API
#include "../gr-dvbs2rx_amd/csrc/c_api_common.h"

// what c_api_core.hip defines in the library; that file binds the LDPC decoder too, which these programs do not link
thread_local std::string dvbs2::g_api_error;
int dvbs2::check_device(int) { return dvbs2::fail(DVBS2_EDEVICE, "this program looks for no device"); }

// "<entry> <code>: <text>" or "<entry> ok"; with an empty entry "refused <code>: <text>" or "ok" (the text is the one c_api_common.h keeps)
inline void answer(const char* entry, int code)
{
    if (code) std::printf("%s%s%d: %s\n", entry, *entry ? " " : "refused ", code, dvbs2::g_api_error.c_str());
    else std::printf("%s%sok\n", entry, *entry ? " " : "");
}
#endif
