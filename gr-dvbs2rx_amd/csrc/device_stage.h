// device_stage.h -- what every host-side stage class (*_hip.h) is built on: the two errors, the device, the plain device buffers
// and the beginning and end of a device method. Host code only. Internal, not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include <vector>
#include "device_guard.h"

namespace dvbs2 {

// hipMemset of device memory for a constructor or a reset. The runtime may return from hipMemset before the device has written: the
// fill is work on the null stream, and a caller's non-blocking stream does not wait for the null stream (measured:
// notes/stream_order.md). The bytes are there when this returns. Not for a work path: it waits on the host.
inline hipError_t memset_done(void* p, int value, size_t bytes)
{
    const hipError_t e = hipMemset(p, value, bytes);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}

enum StageCode { kArgument = -1, kDevice = -2, kSize = -3 }; // what the C ABI answers for a failure (c_api_common.h asserts the values)
struct StageError { // the code is decided where the error is raised; = {} clears
    int code = 0; std::string text; // (code: a StageCode once there is a text)
    void argument(const std::string& t) { code = kArgument; text = t; }
    void device(const std::string& t) { code = kDevice; text = t; }
};

class DeviceStage {
public:
    bool ok() const { return err_.text.empty(); }
    // ok() reports the constructor; a failed call leaves its code and text in error_code() / error() without disabling the handle
    const std::string& error() const { return call_err_.text.empty() ? err_.text : call_err_.text; }
    int error_code() const { return call_err_.text.empty() ? err_.code : call_err_.code; }
    DeviceStage(const DeviceStage&) = delete; DeviceStage& operator=(const DeviceStage&) = delete;

protected:
    explicit DeviceStage(int device) : device_(device) {}
    ~DeviceStage() // (after the derived destructor: nothing of the stage is in flight any more)
    {
        DeviceGuard guard(device_);
        for (void* p : bufs_) (void)hipFree(p);
    }

    // hipMalloc of `count` elements on the current device (the caller holds a DeviceGuard or an Entry); the destructor above frees it.
    // Pinned host memory, events, streams and what outlives the handle are not buffers of this kind and stay with their class.
    template <class T> hipError_t alloc(T** p, size_t count)
    {
        const hipError_t e = hipMalloc(p, count * sizeof(T));
        if (e == hipSuccess) bufs_.push_back(*p);
        return e;
    }

    // Entering a device method: the error of the last call is cleared and the stage's device is current for this object's scope.
    // !ok: the constructor had failed, or hipSetDevice did ("hipSetDevice failed" is then the call's text, unless the method gives its own).
    struct Entry {
        DeviceGuard guard;
        bool ok;
        explicit Entry(DeviceStage& s) : guard(s.device_), ok(s.ok() && guard.ok)
        {
            s.call_err_ = {};
            if (!guard.ok) s.call_err_.device("hipSetDevice failed");
        }
    };

    // e failed: `to` becomes `code` with the text "<what>: <HIP error string>". `what` is always the caller's.
    static bool hip_ok(hipError_t e, const char* what, StageError& to, int code = kDevice)
    {
        if (e != hipSuccess) to = { code, std::string(what) + ": " + hipGetErrorString(e) };
        return e == hipSuccess;
    }
    // after the launches of a method: 0, or -1 with the call's text "<what>: <HIP error string>"
    int launched(const char* what) { return hip_ok(hipGetLastError(), what, call_err_) ? 0 : -1; }

    StageError err_;      // set by the constructor only
    StageError call_err_; // last failed call
    const int device_;

private:
    std::vector<void*> bufs_;
};

// In a constructor (HIP_OK: to err_) and in a method that returns -1 on failure (HIP_RET: to call_err_), both kDevice. The text is the
// call as it is spelled; HIP_OK_AS gives it where the spelling is not the text (alloc() standing for a hipMalloc).
#define HIP_OK_AS(what, x) do { if (!hip_ok((x), what, err_)) return; } while (0)
#define HIP_OK(x) HIP_OK_AS(#x, x)
#define HIP_RET(x) do { if (!hip_ok((x), #x, call_err_)) return -1; } while (0)

} // namespace dvbs2
