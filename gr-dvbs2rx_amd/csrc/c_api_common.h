// c_api_common.h -- what the translation units of the extern "C" boundary (c_api_*.hip, host_pipe.hip) share: the error plumbing, handle
// creation and destruction, the argument checks and the staging of the host-buffer entries. Internal, not installed.
#pragma once
#include "../../include/dvbs2_fec_hip.h"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <new>
#include <string>
#include "device_stage.h"

namespace dvbs2 {
static_assert(kArgument == DVBS2_EINVAL && kDevice == DVBS2_EDEVICE && kSize == DVBS2_ESIZE, "the stage classes record the codes of the C ABI");

extern thread_local std::string g_api_error; // the ONE string behind dvbs2_last_error, defined in c_api_core.hip
inline int fail(int code, const std::string& msg) { g_api_error = msg; return code; }

#define HCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(DVBS2_EDEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define API_TRY try {
#define API_CATCH } catch (const std::exception& e) { return fail(DVBS2_EDEVICE, e.what()); } catch (...) { return fail(DVBS2_EDEVICE, "unknown exception"); }
#define NEED_HANDLE(h) do { if (!(h)) return fail(DVBS2_EINVAL, "null handle"); } while (0)

int check_device(int device); // c_api_core.hip

// What a handle keeps for its host-buffer entries: one stream and up to kBufs device copies of the caller's buffers, all created on first
// use -- a handle that is only driven through the *_device entries allocates nothing here. The handle's struct names the slots in an
// enum that ends in N_SLOTS and asserts N_SLOTS <= kBufs.
struct HostStage {
    static constexpr int kBufs = 6;
    hipStream_t stream = nullptr;
    void* buf[kBufs] = {};
    size_t bytes[kBufs] = {};

    // (DVBS2_EDEVICE is the only failure; what was allocated before it stays until release())
    int ensure(int slot, size_t need)
    {
        if (buf[slot] && bytes[slot] >= need) return DVBS2_OK;
        (void)hipFree(buf[slot]); buf[slot] = nullptr; bytes[slot] = 0;
        const hipError_t e = hipMalloc(&buf[slot], need);
        if (e != hipSuccess) // (the slot number is the handle's enum: which of its buffers)
            return fail(DVBS2_EDEVICE, "hipMalloc of staging buffer " + std::to_string(slot) + " (" + std::to_string(need) + " bytes): " + hipGetErrorString(e));
        bytes[slot] = need;
        return DVBS2_OK;
    }
    template <class T> T* at(int slot) const { return static_cast<T*>(buf[slot]); }
    int sync() { HCHK(hipStreamSynchronize(stream)); return DVBS2_OK; }
    void release() // (under the handle's DeviceGuard)
    {
        for (int i = 0; i < kBufs; i++) { (void)hipFree(buf[i]); buf[i] = nullptr; bytes[i] = 0; }
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};

// Entering a host-buffer entry: the handle's device current for this object's scope, the handle's stream there. rc != 0: return it.
struct HostEntry {
    DeviceGuard guard;
    int rc;
    HostEntry(HostStage& s, int device) : guard(device), rc(guard.ok ? open(s) : fail(DVBS2_EDEVICE, "hipSetDevice failed")) {}
    static int open(HostStage& s) { if (!s.stream) HCHK(hipStreamCreate(&s.stream)); return DVBS2_OK; }
};

// Every stage handle H is { Impl* impl; HostStage stage; int device; } plus what the stage needs.
template <class H> int null_out(H** h)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    return DVBS2_OK;
}

// failed: what a call into h->impl returned (non-zero: it left its code and text in error_code() / error())
template <class H> int impl_rc(const H* h, bool failed) { return failed ? fail(h->impl->error_code(), h->impl->error()) : DVBS2_OK; }

// The create sequence of every handle type H: make() constructs the implementation with new (std::nothrow); !ok(): its constructor failed.
template <class H, class Make> int make_handle(H** h, int device, Make make)
{
    if (int rc = null_out(h)) return rc;
    if (int rc = check_device(device)) return rc;
    H* o = new (std::nothrow) H();
    if (!o) return fail(DVBS2_EDEVICE, "out of memory");
    o->device = device;
    o->impl = make();
    if (!o->impl || !o->impl->ok()) {
        const int rc = o->impl ? impl_rc(o, true) : fail(DVBS2_EINVAL, "out of memory");
        delete o->impl; delete o;
        return rc;
    }
    *h = o;
    return DVBS2_OK;
}

template <class H> void destroy_handle(H* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    h->stage.release();
    delete h->impl;
    delete h;
}

// The checks of an entry that takes n_frames frames: buffers_ok says that every buffer the entry needs for n_frames > 0 is there,
// also_bad is whatever else makes the call a "bad argument" for any n_frames.
template <class H> int check_frames(const H* h, int n_frames, bool buffers_ok, bool also_bad = false)
{
    NEED_HANDLE(h);
    if (n_frames < 0 || (n_frames && !buffers_ok) || also_bad) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->impl->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

// The checks of an entry of a stream stage, the counterpart of check_frames. A count of the call with its cap and their names in the
// texts: every "<name> is negative" (EINVAL) in list order, then every "<name> exceeds <cap_name>" (ESIZE) in list order.
struct Count { int n, cap; const char* name; const char* cap_name; };
inline int check_counts(std::initializer_list<Count> counts)
{
    for (const Count& c : counts)
        if (c.n < 0) return fail(DVBS2_EINVAL, std::string(c.name) + " is negative");
    for (const Count& c : counts)
        if (c.n > c.cap) return fail(DVBS2_ESIZE, std::string(c.name) + " exceeds " + c.cap_name);
    return DVBS2_OK;
}
// the two counts most stream entries take, against the handle's capacities (stream_stage.h); the row count has one name everywhere
template <class H> int check_stream_counts(const H* h, int n, const char* name, const char* cap_name, int n_streams)
{
    return check_counts({ { n, h->impl->max_samples(), name, cap_name }, { n_streams, h->impl->max_streams(), "n_streams", "max_streams" } });
}
inline int check_in_out(const void* in, const void* out)
{
    if (!in) return fail(DVBS2_EINVAL, "in is null");
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    return DVBS2_OK;
}
inline int check_aligned8(const void* in, const void* out) // (device pointers of complex samples)
{
    if (((uintptr_t)in | (uintptr_t)out) & 7) return fail(DVBS2_EINVAL, "in and out must be 8-byte aligned");
    return DVBS2_OK;
}
// An entry with nothing of its own in front of its buffers: the counts, *done (nothing to do: no sample or no row), in and out.
template <class H> int check_stream_call(const H* h, const void* in, int n, const char* name, const char* cap_name, int n_streams, const void* out, bool* done)
{
    *done = false;
    if (int rc = check_stream_counts(h, n, name, cap_name, n_streams)) return rc;
    if (n == 0 || n_streams == 0) { *done = true; return DVBS2_OK; }
    return check_in_out(in, out);
}

} // namespace dvbs2
