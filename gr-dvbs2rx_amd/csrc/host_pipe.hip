// host_pipe.hip -- see host_pipe.h
#include "host_pipe.h"
#include <algorithm>
#include <cstring>

namespace dvbs2 {

bool host_range_page_locked(const void* p, size_t bytes)
{
    if (!p || !bytes) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; } // an ordinary pageable pointer: not an error
    if (a.type != hipMemoryTypeHost) return false;
    void* start = nullptr; size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, const_cast<void*>(p)) != hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, const_cast<void*>(p)) != hipSuccess || !start || !size) {
        (void)hipGetLastError();
        return false;
    }
    const char* lo = (const char*)start; const char* q = (const char*)p;
    return q >= lo && (size_t)(q - lo) + bytes <= size;
}

int host_pipe_init(HostPipe& p)
{
    for (hipStream_t& st : p.stream) if (!st) HCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (!p.copy_stream) HCHK(hipStreamCreateWithFlags(&p.copy_stream, hipStreamNonBlocking));
    for (hipEvent_t& ev : p.in_ready) if (!ev) HCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return DVBS2_OK;
}

void host_pipe_destroy(HostPipe& p)
{
    for (hipStream_t st : p.stream) if (st) (void)hipStreamDestroy(st);
    if (p.copy_stream) (void)hipStreamDestroy(p.copy_stream);
    for (hipEvent_t ev : p.in_ready) if (ev) (void)hipEventDestroy(ev);
    for (void* b : p.pinned) if (b) (void)hipHostFree(b);
}

int host_add_output(HostPipe& p, HostCall& call, int n_frames, const void* dev, void* user, size_t unit_bytes, int frames_per_unit, size_t pinned_bytes)
{
    void*& pinned = p.pinned[call.outs.size()];
    char* land = (char*)user;
    if (user && !host_range_page_locked(user, (size_t)((n_frames + frames_per_unit - 1) / frames_per_unit) * unit_bytes)) {
        if (!pinned) HCHK(hipHostMalloc(&pinned, pinned_bytes));
        land = (char*)pinned;
    }
    call.outs.push_back({ (const char*)dev, (char*)user, land, unit_bytes, frames_per_unit });
    return DVBS2_OK;
}

int host_pipe_run(HostPipe& p, LdpcDecoderHip* dec, const HostCall& call)
{
    const int n_chunks = (int)call.plan.size();
    auto span = [&](const HostOut& o, int c) { // (byte offset, bytes) of chunk c in output o
        const int f0 = call.plan[c].first, nf = call.plan[c].second, per = o.frames_per_unit;
        return std::pair<size_t, size_t>((size_t)(f0 / per) * o.unit_bytes, (size_t)((nf + per - 1) / per) * o.unit_bytes);
    };
    auto copy_out = [&](int c) -> int {
        for (const HostOut& o : call.outs)
            if (o.user) HCHK(hipMemcpyAsync(o.land + span(o, c).first, o.dev + span(o, c).first, span(o, c).second, hipMemcpyDeviceToHost, p.stream[c % kSlots]));
        return DVBS2_OK;
    };
    auto finish = [&](int c) -> int {
        hipStream_t st = p.stream[c % kSlots];
        const int r = dec->finish(c % kSlots);
        if (r < 0) return fail(dec->error_code(), dec->error());
        if (r > 0) { // the LDPC needed rounds beyond the enqueued ones and rewrote its output: what follows it again, and the copies
            if (call.after_ldpc) if (int rc = call.after_ldpc(call.plan[c].first, call.plan[c].second, st)) return rc;
            if (int rc = copy_out(c)) return rc;
        }
        HCHK(hipStreamSynchronize(st));
        for (const HostOut& o : call.outs)
            if (o.land != o.user) std::memcpy(o.user + span(o, c).first, o.land + span(o, c).first, span(o, c).second);
        return DVBS2_OK;
    };
    // (a failure in the middle of the pipeline must not leave chunks in flight or slots busy: the handle stays usable)
    auto run = [&]() -> int {
        for (int c = 0; c < n_chunks; c++) {
            if (c >= kSlots) if (int rc = finish(c - kSlots)) return rc;
            const int f0 = call.plan[c].first, nf = call.plan[c].second;
            hipStream_t st = p.stream[c % kSlots];
            // (pageable input: the runtime stages the copy while the caller waits; the chunk's own stream)
            if (int rc = call.copy_in(c, f0, nf, call.use_copy_stream ? p.copy_stream : st)) return rc;
            if (call.use_copy_stream) {
                HCHK(hipEventRecord(p.in_ready[c % kSlots], p.copy_stream));
                HCHK(hipStreamWaitEvent(st, p.in_ready[c % kSlots], 0));
            } else if (call.shared_input) {
                // (the shared input travelled on chunk 0's stream: the first chunks on the other streams wait for it)
                if (c == 0) HCHK(hipEventRecord(p.in_ready[0], st));
                else if (c < kSlots) HCHK(hipStreamWaitEvent(st, p.in_ready[0], 0));
            }
            if (int rc = call.enqueue(c, f0, nf, st)) return rc;
            if (call.after_ldpc) if (int rc = call.after_ldpc(f0, nf, st)) return rc;
            if (int rc = copy_out(c)) return rc;
        }
        for (int c = std::max(0, n_chunks - kSlots); c < n_chunks; c++) if (int rc = finish(c)) return rc;
        return DVBS2_OK;
    };
    const int rc = run();
    if (rc != DVBS2_OK) { // nothing of this call stays in flight (copies into the caller's buffers included)
        const std::string keep = g_api_error;
        dec->abort_all();
        (void)hipStreamSynchronize(p.copy_stream);
        for (hipStream_t st : p.stream) (void)hipStreamSynchronize(st);
        g_api_error = keep;
    }
    return rc;
}

} // namespace dvbs2
