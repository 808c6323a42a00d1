// stream_stage.h -- what the stream stage classes (agc, awgn, iqconv, symsync, pulse, resamp, spectrum, ddc, pfbch, pfbsyn) have in common on top
// of DeviceStage: the two capacities of a handle, the check of a caller's taps, and device buffers that start as zeros and that reset()
// zeroes again. Host code only (what their kernels share is in stream_device.hpp). Internal, not installed. The range texts of the
// capacities differ per stage and stay in its check_args.
#pragma once
#include <cmath>
#include <string>
#include <utility>
#include <vector>
#include "device_stage.h"

namespace dvbs2 {

// Host only. n values at v: "null <name>", "<name>[i] is not finite" for the first such i, or empty. (Where null is legal the caller asks.)
inline std::string check_taps(const float* v, int n, const char* name)
{
    if (!v) return std::string("null ") + name;
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return std::string(name) + "[" + std::to_string(i) + "] is not finite";
    return "";
}

class StreamStage : public DeviceStage {
public:
    int max_streams() const { return max_streams_; } // rows of a call at most
    int max_samples() const { return max_samples_; } // elements of a row at most

protected:
    StreamStage(int max_streams, int max_samples, int device) : DeviceStage(device), max_streams_(max_streams), max_samples_(max_samples) {}

    // alloc() of `count` elements that start as zeros; zero(p) makes them zeros again, so the size is written once. The first failure is
    // returned: the allocation's or the fill's (memset_done: the zeros are on the device when it returns).
    template <class T> hipError_t alloc_zeroed(T** p, size_t count)
    {
        const hipError_t e = alloc(p, count);
        if (e != hipSuccess) return e;
        zeroed_.emplace_back(*p, count * sizeof(T));
        return zero(*p);
    }
    hipError_t zero(const void* p)
    {
        for (const auto& z : zeroed_)
            if (z.first == p) return memset_done(z.first, 0, z.second);
        return hipErrorInvalidValue; // not a buffer of alloc_zeroed
    }

    const int max_streams_, max_samples_;

private:
    std::vector<std::pair<void*, size_t>> zeroed_;
};

} // namespace dvbs2
