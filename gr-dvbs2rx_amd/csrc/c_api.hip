// c_api.hip -- extern "C" boundary (include/dvbs2_fec_hip.h). No exceptions leave this file.
#include "../../include/dvbs2_fec_hip.h"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "fec_tables.h"
#include "ldpc_hip.h"
#include "ldpc_schedule.h"
#include "bch_hip.h"
#include "demap_hip.h"
#include "plpayload_hip.h"
#include "plframe_hip.h"
#include "plsync_hip.h"
#include "plcoarse_hip.h"
#include "rotator_hip.h"
#include "symsync_hip.h"
#include "bbdeheader_hip.h"
#include "device_guard.h"
#include "demap_math.hpp"
#include "host_plan.h"
#include <algorithm>
#include <functional>

using namespace dvbs2;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(DVBS2_EDEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define API_TRY try {
#define API_CATCH } catch (const std::exception& e) { return fail(DVBS2_EDEVICE, e.what()); } catch (...) { return fail(DVBS2_EDEVICE, "unknown exception"); }

// Is [p, p + bytes) ONE page-locked host range the copy engine can address (hipHostMalloc'ed, or registered with dvbs2_host_register /
// hipHostRegister)? Decided from the runtime's own record of the allocation that holds p -- its start and size
// (HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR / RANGE_SIZE) must cover the last byte -- so two registrations with a pageable hole between
// them are not mistaken for one. When the runtime cannot answer, the range counts as pageable: the call then stages through the
// handle's own pinned buffers, which is always correct.
static bool host_range_page_locked(const void* p, size_t bytes)
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

static int check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DVBS2_EDEVICE, "no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(DVBS2_EINVAL, "device index out of range");
    return DVBS2_OK;
}

// The create sequence of every handle type H: make(o) constructs the implementation with new (std::nothrow), stores it in o and returns it.
// A constructor that failed says so through ok() / error(): DVBS2_EINVAL, or, where hip_is_edevice, DVBS2_EDEVICE when the text names a hip call.
template <class H, class Make> static int make_handle(H** h, int device, bool hip_is_edevice, Make make)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    if (int rc = check_device(device)) return rc;
    H* o = new (std::nothrow) H();
    if (!o) return fail(DVBS2_EDEVICE, "out of memory");
    o->device = device;
    auto* impl = make(o);
    if (!impl || !impl->ok()) {
        const std::string msg = impl ? impl->error() : "out of memory";
        delete impl; delete o;
        return fail(hip_is_edevice && msg.find("hip") != std::string::npos ? DVBS2_EDEVICE : DVBS2_EINVAL, msg);
    }
    *h = o;
    return DVBS2_OK;
}

static int host_chunk_env() { const char* e = getenv("DVBS2_HOST_CHUNK"); return e ? std::max(2, atoi(e)) : 0; } // 0: unset

/* ------------------------------------------------------------------ chunked host pipeline (dvbs2_ldpc_decode, dvbs2_chain_decode[_llr]) */
constexpr int kSlots = LdpcDecoderHip::kSlots;

// what a handle keeps for its host-buffer entry, created on first use
struct HostPipe {
    hipStream_t stream[kSlots] = {}; // one per chunk slot, so that the transfer of chunk c + 1 runs under the decode of chunk c
    // inputs go through ONE copy stream, chunk after chunk (each copy at the full link rate, chunk 0 first), and the chunk's compute
    // stream waits for its event: with the copies on the four compute streams a page-locked caller's chunks 0..3 shared the link and
    // the first kernel started after FOUR chunks had arrived instead of one (round 3: page-locked callers 8 % slower than pageable ones)
    hipStream_t copy_stream = nullptr;
    hipEvent_t in_ready[kSlots] = {};
    // pinned landing buffers for the outputs (in the order of HostCall::outs): a device-to-host copy into pageable memory blocks the
    // calling thread until the chunk's kernels are done, which would serialise the chunks
    void* pinned[3] = {};
};

static int host_pipe_init(HostPipe& p)
{
    for (hipStream_t& st : p.stream) if (!st) HCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (!p.copy_stream) HCHK(hipStreamCreateWithFlags(&p.copy_stream, hipStreamNonBlocking));
    for (hipEvent_t& ev : p.in_ready) if (!ev) HCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return DVBS2_OK;
}

static void host_pipe_destroy(HostPipe& p) // (under the handle's DeviceGuard)
{
    for (hipStream_t st : p.stream) if (st) (void)hipStreamDestroy(st);
    if (p.copy_stream) (void)hipStreamDestroy(p.copy_stream);
    for (hipEvent_t ev : p.in_ready) if (ev) (void)hipEventDestroy(ev);
    for (void* b : p.pinned) if (b) (void)hipHostFree(b);
}

// one output of a call, from the device staging `dev` to `user` (null: not asked for) by way of `land`: one unit of `unit_bytes` per
// `frames_per_unit` frames (1, or the LDPC group size for the decoder's return words)
struct HostOut { const char* dev; char* user; char* land; size_t unit_bytes; int frames_per_unit; };

// what one call hands to host_pipe_run; the callables enqueue on the stream they are given and return a DVBS2_* code
struct HostCall {
    std::vector<std::pair<int, int>> plan; // host_chunk_plan()
    std::vector<HostOut> outs;             // host_add_output(); fetched in this order
    bool use_copy_stream = false;          // inputs through the copy stream + event (page-locked input), else on the chunk's own stream
    bool shared_input = false;             // chunk 0's copy_in also brings an input that every chunk reads (the chain's single N0)
    std::function<int(int c, int f0, int nf, hipStream_t cs)> copy_in;
    std::function<int(int c, int f0, int nf, hipStream_t st)> enqueue; // up to and including the LDPC decode in slot c % kSlots
    std::function<int(int f0, int nf, hipStream_t st)> after_ldpc;     // what follows it on the stream (may be empty); again after extra rounds
};

// Results land where the DMA engine can write them: straight in the caller's buffer when it is page-locked (hipHostMalloc'ed, or
// registered once with dvbs2_host_register -- what a block does with its item buffers; the WHOLE range has to lie inside one allocation
// / registration: host_range_page_locked), else in a pinned buffer of the handle (pinned_bytes: for max_frames) that is copied out when
// the chunk has finished.
static int host_add_output(HostPipe& p, HostCall& call, int n_frames, const void* dev, void* user, size_t unit_bytes, int frames_per_unit, size_t pinned_bytes)
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

// The pipeline: chunk c of the plan uses slot and stream c % kSlots (its own range of the decoder's state and message buffers); its input
// copy runs under the kernels of chunk c - 1 and its results go back while chunk c + 1 decodes.
static int host_pipe_run(HostPipe& p, LdpcDecoderHip* dec, const HostCall& call)
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
        if (r < 0) return fail(DVBS2_EDEVICE, dec->error());
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
        const std::string keep = g_err;
        dec->abort_all();
        (void)hipStreamSynchronize(p.copy_stream);
        for (hipStream_t st : p.stream) (void)hipStreamSynchronize(st);
        g_err = keep;
    }
    return rc;
}

struct dvbs2_ldpc {
    LdpcDecoderHip* dec = nullptr;
    // host staging (dvbs2_ldpc_decode): device copies of the caller's buffers, the pipeline's streams and pinned buffers
    int8_t* d_in = nullptr; uint8_t* d_bits = nullptr; int8_t* d_llr = nullptr; int32_t* d_ret = nullptr;
    HostPipe pipe;
    int device = 0;
    // experiment / test knobs of the host entry, read ONCE when the handle is created (no getenv per decode call)
    std::string host_plan;      // DVBS2_HOST_PLAN: comma list of chunk sizes, the last one repeats
    int host_chunk = 0;         // DVBS2_HOST_CHUNK: one chunk size for the whole call (0: the measured plan)
    int host_copy_stream = -1;  // DVBS2_HOST_COPY_STREAM: 0 / 1 force the copies off / onto the copy stream (-1: by kind of input buffer)
};

extern "C" {

const char* dvbs2_last_error(void) { return g_err.c_str(); }

int dvbs2_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dvbs2_host_register(void* p, size_t bytes)
{
    if (!p || !bytes) return fail(DVBS2_EINVAL, "bad argument");
    HCHK(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return DVBS2_OK;
}

int dvbs2_host_is_page_locked(const void* p, size_t bytes) { return host_range_page_locked(p, bytes) ? 1 : 0; }

int dvbs2_host_alloc(void** p, size_t bytes)
{
    if (!p || !bytes) return fail(DVBS2_EINVAL, "bad argument");
    *p = nullptr;
    HCHK(hipHostMalloc(p, bytes, hipHostMallocDefault));
    return DVBS2_OK;
}

int dvbs2_host_free(void* p)
{
    if (!p) return DVBS2_OK;
    HCHK(hipHostFree(p));
    return DVBS2_OK;
}

int dvbs2_host_unregister(void* p)
{
    if (!p) return fail(DVBS2_EINVAL, "bad argument");
    HCHK(hipHostUnregister(p));
    return DVBS2_OK;
}

int dvbs2_get_fec_info(int standard, int framesize, int rate, dvbs2_fec_info_t* out)
{
    if (!out) return fail(DVBS2_EINVAL, "null out");
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    std::memset(out, 0, sizeof(*out));
    out->bch_k = fi.bch_k; out->bch_n = fi.bch_n; out->bch_t = fi.bch_t;
    out->ldpc_k = fi.ldpc_k; out->ldpc_n = fi.ldpc_n;
    if (fi.table) { out->table_k = fi.table->K; std::strncpy(out->table, fi.table->name, sizeof(out->table) - 1); }
    return DVBS2_OK;
}

const char* dvbs2_rate_name(int rate) { return rate_name(rate); }
int dvbs2_rate_from_name(const char* name)
{
    if (!name) return -1;
    for (int r = 0; r < num_rates(); r++) if (!std::strcmp(rate_name(r), name)) return r;
    return -1;
}

const char* dvbs2_ldpc_table_name(int index)
{
    const LdpcTableDesc* t = ldpc_table_at(index);
    return t ? t->name : nullptr;
}

int dvbs2_ldpc_table_info(const char* table, int* n, int* k, int* q, int* links_total, int* conflict_layers)
{
    API_TRY
    LdpcSchedule s;
    if (!compile_ldpc_schedule(find_ldpc_table(table), &s)) return fail(DVBS2_EINVAL, "unknown LDPC table");
    if (n) *n = s.N; if (k) *k = s.K; if (q) *q = s.q;
    if (links_total) *links_total = s.links_total;
    if (conflict_layers) *conflict_layers = s.conflict_layers;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_ldpc_layer_info(const char* table, int layer, int* block, int* groups, int* shifts, int max_entries)
{
    API_TRY
    LdpcSchedule s;
    if (!compile_ldpc_schedule(find_ldpc_table(table), &s)) return fail(DVBS2_EINVAL, "unknown LDPC table");
    if (layer < 0 || layer >= s.q) return fail(DVBS2_EINVAL, "layer out of range");
    const LdpcLayer& L = s.layers[layer];
    if (block) *block = L.block;
    for (int e = 0; e < L.cnt && e < max_entries; e++) {
        const LdpcEntry& en = s.entries[L.entry_off + e];
        if (groups) groups[e] = en.base / 360;
        if (shifts) shifts[e] = (360 - en.rot) % 360;
    }
    return L.cnt;
    API_CATCH
}

static int ldpc_make(dvbs2_ldpc_t** h, const LdpcTableDesc* t, int message_bits, int G, int max_frames, int device)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    if (!t) return fail(DVBS2_EINVAL, "unknown LDPC table");
    return make_handle(h, device, true, [&](dvbs2_ldpc* o) {
        if (const char* e = getenv("DVBS2_HOST_PLAN")) o->host_plan = e;
        o->host_chunk = host_chunk_env();
        if (const char* e = getenv("DVBS2_HOST_COPY_STREAM")) o->host_copy_stream = atoi(e) != 0 ? 1 : 0;
        return o->dec = new (std::nothrow) LdpcDecoderHip(t, message_bits, G, max_frames, device);
    });
}

int dvbs2_ldpc_create(dvbs2_ldpc_t** h, int standard, int framesize, int rate, int group_size, int max_frames, int device)
{
    API_TRY
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi) || !fi.table) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return ldpc_make(h, fi.table, (int)fi.ldpc_k, group_size, max_frames, device);
    API_CATCH
}

int dvbs2_ldpc_create_table(dvbs2_ldpc_t** h, const char* table, int message_bits, int group_size, int max_frames, int device)
{
    API_TRY
    return ldpc_make(h, find_ldpc_table(table), message_bits, group_size, max_frames, device);
    API_CATCH
}

void dvbs2_ldpc_destroy(dvbs2_ldpc_t* h)
{
    if (!h) return;
    DeviceGuard g(h->device);
    (void)hipFree(h->d_in); (void)hipFree(h->d_bits); (void)hipFree(h->d_llr); (void)hipFree(h->d_ret);
    host_pipe_destroy(h->pipe);
    delete h->dec;
    delete h;
}

int dvbs2_ldpc_params(const dvbs2_ldpc_t* h, int* n, int* table_k, int* message_bits, int* q, int* group_size)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n) *n = h->dec->N(); if (table_k) *table_k = h->dec->K();
    if (message_bits) *message_bits = h->dec->out_bits_message();
    if (q) *q = h->dec->q(); if (group_size) *group_size = h->dec->group_size();
    return DVBS2_OK;
}

static int ldpc_check_args(dvbs2_ldpc_t* h, const void* in, int n_frames, int max_trials, int out_mode, const void* bits,
                           const void* d_llr_out = nullptr, bool device_pointers = false)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && (!in || !bits))) return fail(DVBS2_EINVAL, "bad argument");
    // the kernels move LLRs with 8-byte loads and stores (include/dvbs2_fec_hip.h): a misaligned device pointer would be a GPU memory fault
    if (device_pointers && ((((uintptr_t)in) | ((uintptr_t)d_llr_out)) & 7u)) return fail(DVBS2_EINVAL, "d_llr_in / d_llr_out must be 8-byte aligned");
    if (out_mode != DVBS2_OM_CODEWORD && out_mode != DVBS2_OM_MESSAGE) return fail(DVBS2_EINVAL, "bad out_mode");
    if (n_frames > h->dec->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

int dvbs2_ldpc_decode_device(dvbs2_ldpc_t* h, const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode,
                             uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret, void* stream)
{
    API_TRY
    if (int rc = ldpc_check_args(h, d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, true)) return rc;
    if (h->dec->decode_device(d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, d_ret, (hipStream_t)stream))
        return fail(DVBS2_EDEVICE, h->dec->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_ldpc_enqueue_device(dvbs2_ldpc_t* h, const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode,
                              uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret, void* stream)
{
    API_TRY
    if (int rc = ldpc_check_args(h, d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, true)) return rc;
    if (h->dec->enqueue(d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, d_ret, (hipStream_t)stream, 0, 0))
        return fail(DVBS2_EDEVICE, h->dec->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_ldpc_finish(dvbs2_ldpc_t* h)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->dec->finish(0) < 0) return fail(DVBS2_EDEVICE, h->dec->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_ldpc_decode(dvbs2_ldpc_t* h, const int8_t* llr_in, int n_frames, int max_trials, int out_mode,
                      uint8_t* bits_out, int8_t* llr_out, int32_t* ret)
{
    API_TRY
    if (int rc = ldpc_check_args(h, llr_in, n_frames, max_trials, out_mode, bits_out)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    LdpcDecoderHip* dec = h->dec;
    const size_t N = dec->N(), mf = dec->max_frames();
    const int G = dec->group_size();
    const size_t ret_bytes = ((mf + G - 1) / G + kSlots) * 4;
    if (int rc = host_pipe_init(h->pipe)) return rc;
    if (!h->d_in) HCHK(hipMalloc(&h->d_in, mf * N));
    if (!h->d_bits) HCHK(hipMalloc(&h->d_bits, mf * (N / 8)));
    if (!h->d_llr) HCHK(hipMalloc(&h->d_llr, mf * N));
    if (!h->d_ret) HCHK(hipMalloc(&h->d_ret, ret_bytes));
    const size_t out_bytes = (out_mode ? dec->out_bits_message() : (int)N) / 8;
    HostCall call;
    if (int rc = host_add_output(h->pipe, call, n_frames, h->d_bits, bits_out, out_bytes, 1, mf * (N / 8))) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, h->d_llr, llr_out, N, 1, mf * N)) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, h->d_ret, ret, 4, G, ret_bytes)) return rc;
    const bool in_locked = host_range_page_locked(llr_in, (size_t)n_frames * N);
    call.plan = host_chunk_plan(n_frames, G, in_locked, false, h->host_chunk, h->host_plan);
    call.use_copy_stream = h->host_copy_stream >= 0 ? h->host_copy_stream != 0 : in_locked; // (DVBS2_HOST_COPY_STREAM: experiments)
    call.copy_in = [&](int, int f0, int nf, hipStream_t cs) -> int {
        HCHK(hipMemcpyAsync(h->d_in + (size_t)f0 * N, llr_in + (size_t)f0 * N, (size_t)nf * N, hipMemcpyHostToDevice, cs));
        return DVBS2_OK;
    };
    call.enqueue = [&](int c, int f0, int nf, hipStream_t st) -> int {
        if (dec->enqueue(h->d_in + (size_t)f0 * N, nf, max_trials, out_mode, h->d_bits + (size_t)f0 * out_bytes,
                         llr_out ? h->d_llr + (size_t)f0 * N : nullptr, h->d_ret + f0 / G, st, c % kSlots, f0))
            return fail(DVBS2_EDEVICE, dec->error());
        return DVBS2_OK;
    };
    return host_pipe_run(h->pipe, dec, call); // (nothing after the LDPC: outputs that extra rounds rewrote are only fetched again)
    API_CATCH
}

const char* dvbs2_ldpc_kernel_name(const dvbs2_ldpc_t* h)
{
    return h ? h->dec->kernel_name() : nullptr;
}

int dvbs2_ldpc_fallback_rounds(const dvbs2_ldpc_t* h)
{
    return h ? h->dec->fallback_rounds() : -1;
}

int dvbs2_measure_host_copy(int device, size_t bytes, int n_streams, int kind, double* h2d_gbs, double* d2h_gbs)
{
    API_TRY
    if (!bytes || n_streams < 1 || n_streams > 16 || kind < 0 || kind > 2) return fail(DVBS2_EINVAL, "bad argument");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    void* host = nullptr; void* dev = nullptr;
    hipStream_t st[16] = {};
    hipEvent_t e0 = nullptr, e1 = nullptr, done[16] = {};
    int rc = DVBS2_OK;
    bool registered = false;
    auto body = [&]() -> int {
        if (kind == 0) HCHK(hipHostMalloc(&host, bytes));
        else if (kind == 1) {
            // a mapping of its own for the registration (whole pages nothing else lives in; shared anonymous memory: no copy-on-write, no
            // anonymous huge pages under it) -- see dvbs2_host_alloc in the header for why heap memory is not registered here any more
            host = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
            if (host == MAP_FAILED) { host = nullptr; return fail(DVBS2_EDEVICE, "out of host memory"); }
            std::memset(host, 1, bytes);
            HCHK(hipHostRegister(host, bytes, hipHostRegisterDefault));
            registered = true;
        } else {
            host = std::malloc(bytes);
            if (!host) return fail(DVBS2_EDEVICE, "out of host memory");
            std::memset(host, 1, bytes);
        }
        HCHK(hipMalloc(&dev, bytes));
        for (int i = 0; i < n_streams; i++) { HCHK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking)); HCHK(hipEventCreateWithFlags(&done[i], hipEventDisableTiming)); }
        HCHK(hipEventCreate(&e0)); HCHK(hipEventCreate(&e1));
        const size_t part = (bytes / n_streams) & ~(size_t)4095;
        for (int dir = 0; dir < 2; dir++) {
            double best = 0;
            for (int rep = 0; rep < 3; rep++) { // first repetition warms the path
                HCHK(hipDeviceSynchronize());
                HCHK(hipEventRecord(e0, st[0]));
                for (int i = 1; i < n_streams; i++) HCHK(hipStreamWaitEvent(st[i], e0, 0));
                for (int i = 0; i < n_streams; i++) {
                    char* hp = (char*)host + (size_t)i * part; char* dp = (char*)dev + (size_t)i * part;
                    if (dir == 0) HCHK(hipMemcpyAsync(dp, hp, part, hipMemcpyHostToDevice, st[i]));
                    else HCHK(hipMemcpyAsync(hp, dp, part, hipMemcpyDeviceToHost, st[i]));
                    if (i) { HCHK(hipEventRecord(done[i], st[i])); HCHK(hipStreamWaitEvent(st[0], done[i], 0)); }
                }
                HCHK(hipEventRecord(e1, st[0]));
                HCHK(hipEventSynchronize(e1));
                float ms = 0; HCHK(hipEventElapsedTime(&ms, e0, e1));
                if (rep && ms > 0) best = std::max(best, (double)part * n_streams / (ms * 1e-3) / 1e9);
            }
            if (dir == 0) { if (h2d_gbs) *h2d_gbs = best; } else if (d2h_gbs) *d2h_gbs = best;
        }
        return DVBS2_OK;
    };
    rc = body();
    (void)hipDeviceSynchronize();
    for (int i = 0; i < n_streams; i++) { if (st[i]) (void)hipStreamDestroy(st[i]); if (done[i]) (void)hipEventDestroy(done[i]); }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (dev) (void)hipFree(dev);
    if (host) {
        if (kind == 0) (void)hipHostFree(host);
        else if (kind == 1) { if (registered) (void)hipHostUnregister(host); (void)munmap(host, bytes); }
        else std::free(host);
    }
    return rc;
    API_CATCH
}

} // extern "C"

// every SIMD of the device busy with dependent VALU adds; workgroup 0 reports its s_memtime (shader clock) and s_memrealtime (100 MHz) deltas
__global__ void dvbs2_clock_probe_kernel(unsigned long long* out, int n)
{
    unsigned long long r0, r1;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0));
    const unsigned long long t0 = __builtin_readcyclecounter();
    uint32_t a = threadIdx.x;
    for (int i = 0; i < n; i++) asm volatile("v_add_u32 %0, %0, 1\n\tv_add_u32 %0, %0, 1\n\tv_add_u32 %0, %0, 1\n\tv_add_u32 %0, %0, 1" : "+v"(a));
    const unsigned long long t1 = __builtin_readcyclecounter();
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1));
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; out[2] = a; }
}

extern "C" {

int dvbs2_measure_shader_clock(int device, double* ghz, double* kernel_ms)
{
    API_TRY
    if (!ghz) return fail(DVBS2_EINVAL, "bad argument");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    unsigned long long* d = nullptr; unsigned long long hv[3] = {};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0;
    auto body = [&]() -> int {
        HCHK(hipMalloc(&d, 64));
        HCHK(hipEventCreate(&e0)); HCHK(hipEventCreate(&e1));
        for (int rep = 0; rep < 2; rep++) { // (the first launch lets the clock ramp)
            HCHK(hipEventRecord(e0, nullptr));
            hipLaunchKernelGGL(dvbs2_clock_probe_kernel, dim3(2048), dim3(256), 0, nullptr, d, 300000);
            HCHK(hipEventRecord(e1, nullptr));
            HCHK(hipEventSynchronize(e1));
        }
        HCHK(hipEventElapsedTime(&ms, e0, e1));
        HCHK(hipMemcpy(hv, d, 24, hipMemcpyDeviceToHost));
        return DVBS2_OK;
    };
    const int rc = body();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (rc != DVBS2_OK) return rc;
    if (!hv[1]) return fail(DVBS2_EDEVICE, "clock probe returned nothing");
    *ghz = (double)hv[0] / (double)hv[1] * 0.1; // s_memrealtime counts at 100 MHz
    if (kernel_ms) *kernel_ms = ms;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_debug_cu_slot_table(int device, int device_key, unsigned long long* table_address, int* nonzero_words)
{
    API_TRY
    if (!table_address) return fail(DVBS2_EINVAL, "bad argument");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    std::string e;
    int* t = cu_slot_table(device_key, &e);
    if (!t) return fail(DVBS2_EDEVICE, e);
    *table_address = (unsigned long long)(uintptr_t)t;
    if (nonzero_words) {
        std::vector<int> hv(kCuSlots);
        HCHK(hipMemcpy(hv.data(), t, hv.size() * 4, hipMemcpyDeviceToHost));
        int nz = 0;
        for (int v : hv) nz += v != 0;
        *nonzero_words = nz;
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_ldpc_profile(dvbs2_ldpc_t* h, int enable, double* total_ms, int* launches)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (total_ms) *total_ms = h->dec->profile_ms();
    if (launches) *launches = h->dec->profile_launches();
    h->dec->set_profiling(enable != 0);
    if (enable) h->dec->reset_profile();
    return DVBS2_OK;
}

} // extern "C"

/* ------------------------------------------------------------------ BCH */
struct dvbs2_bch {
    BchDecoderHip* dec = nullptr;
    uint8_t* d_cw = nullptr; uint8_t* d_msg = nullptr; int32_t* d_corr = nullptr;
    hipStream_t stream = nullptr;
    int device = 0;
};

static int bch_make(dvbs2_bch_t** h, int m, uint32_t prim_poly, int t, int n, int max_frames, int device)
{
    return make_handle(h, device, true, [&](dvbs2_bch* o) { return o->dec = new (std::nothrow) BchDecoderHip(m, prim_poly, t, n, max_frames, device); });
}

static void bch_field(int framesize, int* m, uint32_t* prim)
{   // reference lib/bch_decoder_bb_impl.cc:58-63
    if (framesize == DVBS2_FECFRAME_NORMAL) { *m = 16; *prim = 0x1002Du; }      // x^16 + x^5 + x^3 + x^2 + 1
    else if (framesize == DVBS2_FECFRAME_SHORT) { *m = 14; *prim = 0x402Bu; }   // x^14 + x^5 + x^3 + x + 1
    else { *m = 15; *prim = 0x802Du; }                                           // x^15 + x^5 + x^3 + x^2 + 1
}

extern "C" {

int dvbs2_bch_create(dvbs2_bch_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    int m; uint32_t prim;
    bch_field(framesize, &m, &prim);
    int rc = bch_make(h, m, prim, (int)fi.bch_t, (int)fi.bch_n, max_frames, device);
    if (rc == DVBS2_OK && (*h)->dec->code().k != (int)fi.bch_k) { dvbs2_bch_destroy(*h); *h = nullptr; return fail(DVBS2_EINVAL, "BCH k mismatch with the parameter table"); }
    return rc;
    API_CATCH
}

int dvbs2_bch_create_raw(dvbs2_bch_t** h, int m, uint32_t prim_poly, int t, int n, int max_frames, int device)
{
    API_TRY
    return bch_make(h, m, prim_poly, t, n, max_frames, device);
    API_CATCH
}

void dvbs2_bch_destroy(dvbs2_bch_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_cw); (void)hipFree(h->d_msg); (void)hipFree(h->d_corr);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->dec;
    delete h;
}

int dvbs2_bch_params(const dvbs2_bch_t* h, int* n, int* k, int* t)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n) *n = h->dec->code().n; if (k) *k = h->dec->code().k; if (t) *t = h->dec->code().t;
    return DVBS2_OK;
}

int dvbs2_bch_genpoly(const dvbs2_bch_t* h, uint8_t* gen, int max_coefs)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    const auto& g = h->dec->code().gen;
    if (gen) for (int i = 0; i < (int)g.size() && i < max_coefs; i++) gen[i] = g[i];
    return h->dec->code().gdeg;
}

int dvbs2_bch_set_descramble(dvbs2_bch_t* h, int enable)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->dec->set_descramble(enable != 0)) return fail(DVBS2_EDEVICE, h->dec->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bb_descramble_sequence(uint8_t* seq, int n_bytes)
{
    if (!seq || n_bytes < 0 || n_bytes > 64800 / 8) return fail(DVBS2_EINVAL, "bad argument");
    bb_derandomise_sequence(seq, n_bytes);
    return DVBS2_OK;
}

int dvbs2_bch_decode_device(dvbs2_bch_t* h, const uint8_t* d_cw, int n_frames, uint8_t* d_msg, int32_t* d_corr, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!d_cw || !d_msg || !d_corr))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dec->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->dec->decode_device(d_cw, n_frames, d_msg, d_corr, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->dec->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bch_decode(dvbs2_bch_t* h, const uint8_t* cw, int n_frames, uint8_t* msg, int32_t* corrections)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!cw || !msg || !corrections))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dec->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const size_t nb = h->dec->code().n / 8, kb = h->dec->code().k / 8, mf = h->dec->max_frames();
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_cw) HCHK(hipMalloc(&h->d_cw, mf * nb));
    if (!h->d_msg) HCHK(hipMalloc(&h->d_msg, mf * kb));
    if (!h->d_corr) HCHK(hipMalloc(&h->d_corr, mf * 4));
    HCHK(hipMemcpyAsync(h->d_cw, cw, (size_t)n_frames * nb, hipMemcpyHostToDevice, h->stream));
    if (h->dec->decode_device(h->d_cw, n_frames, h->d_msg, h->d_corr, h->stream)) return fail(DVBS2_EDEVICE, h->dec->error());
    HCHK(hipMemcpyAsync(msg, h->d_msg, (size_t)n_frames * kb, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipMemcpyAsync(corrections, h->d_corr, (size_t)n_frames * 4, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ demapper */
struct dvbs2_demap {
    DemapperHip* dm = nullptr;
    float* d_syms = nullptr; float* d_n0 = nullptr; int8_t* d_llr = nullptr; float* d_snr = nullptr;
    hipStream_t stream = nullptr;
    int device = 0;
};

extern "C" {

int dvbs2_demap_create(dvbs2_demap_t** h, int framesize, int rate, int constellation, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, false, [&](dvbs2_demap* o) { return o->dm = new (std::nothrow) DemapperHip(framesize, rate, constellation, max_frames, device); });
    API_CATCH
}

void dvbs2_demap_destroy(dvbs2_demap_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_syms); (void)hipFree(h->d_n0); (void)hipFree(h->d_llr); (void)hipFree(h->d_snr);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->dm;
    delete h;
}

int dvbs2_apsk_points(int constellation, int rate, float* re_im)
{
    if (!re_im) return fail(DVBS2_EINVAL, "bad argument");
    if (constellation != DVBS2_MOD_16APSK && constellation != DVBS2_MOD_32APSK) return fail(DVBS2_EINVAL, "Unsupported constellation");
    if (!apsk_points(constellation, rate, re_im)) return fail(DVBS2_EINVAL, "Unsupported code rate for 16APSK / 32APSK");
    return DVBS2_OK;
}

int dvbs2_demap_params(const dvbs2_demap_t* h, int* n_syms, int* n_llr, int* n_mod, int* column_order)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms) *n_syms = h->dm->n_syms(); if (n_llr) *n_llr = h->dm->n_llr();
    if (n_mod) *n_mod = h->dm->n_mod(); if (column_order) *column_order = h->dm->column_order();
    return DVBS2_OK;
}

int dvbs2_demap_soft_device(dvbs2_demap_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count, int8_t* d_llr_out, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!d_syms || !d_n0 || !d_llr_out)) || (n0_count != 1 && n0_count != n_frames)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dm->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->dm->soft_device(d_syms, n_frames, d_n0, n0_count, d_llr_out, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->dm->error());
    return DVBS2_OK;
    API_CATCH
}

static int demap_stage(dvbs2_demap_t* h, const float* syms, int n_frames)
{
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const size_t mf = h->dm->max_frames(), ns = h->dm->n_syms();
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_syms) HCHK(hipMalloc(&h->d_syms, mf * ns * 8));
    if (!h->d_n0) HCHK(hipMalloc(&h->d_n0, mf * 4));
    if (!h->d_llr) HCHK(hipMalloc(&h->d_llr, mf * h->dm->n_llr()));
    if (!h->d_snr) HCHK(hipMalloc(&h->d_snr, mf * 4));
    HCHK(hipMemcpyAsync(h->d_syms, syms, (size_t)n_frames * ns * 8, hipMemcpyHostToDevice, h->stream));
    return DVBS2_OK;
}

int dvbs2_demap_soft(dvbs2_demap_t* h, const float* syms, int n_frames, const float* n0, int n0_count, int8_t* llr_out)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!syms || !n0 || !llr_out)) || (n0_count != 1 && n0_count != n_frames)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dm->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames == 0) return DVBS2_OK;
    if (int rc = demap_stage(h, syms, n_frames)) return rc;
    HCHK(hipMemcpyAsync(h->d_n0, n0, (size_t)n0_count * 4, hipMemcpyHostToDevice, h->stream));
    if (h->dm->soft_device(h->d_syms, n_frames, h->d_n0, n0_count, h->d_llr, h->stream)) return fail(DVBS2_EDEVICE, h->dm->error());
    HCHK(hipMemcpyAsync(llr_out, h->d_llr, (size_t)n_frames * h->dm->n_llr(), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_demap_estimate_snr_device(dvbs2_demap_t* h, const float* d_syms, int n_frames, float* d_snr_lin, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!d_syms || !d_snr_lin))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dm->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->dm->snr_device(d_syms, nullptr, n_frames, d_snr_lin, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->dm->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_demap_estimate_snr(dvbs2_demap_t* h, const float* syms, int n_frames, float* snr_lin)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!syms || !snr_lin))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dm->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames == 0) return DVBS2_OK;
    if (int rc = demap_stage(h, syms, n_frames)) return rc;
    if (h->dm->snr_device(h->d_syms, nullptr, n_frames, h->d_snr, h->stream)) return fail(DVBS2_EDEVICE, h->dm->error());
    HCHK(hipMemcpyAsync(snr_lin, h->d_snr, (size_t)n_frames * 4, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_demap_refine_snr_device(dvbs2_demap_t* h, const float* d_syms, const int8_t* d_ref_llr, int n_frames, float* d_snr_lin, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!d_syms || !d_ref_llr || !d_snr_lin))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dm->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->dm->snr_device(d_syms, d_ref_llr, n_frames, d_snr_lin, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->dm->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_demap_refine_snr(dvbs2_demap_t* h, const float* syms, const int8_t* ref_llr, int n_frames, float* snr_lin)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!syms || !ref_llr || !snr_lin))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->dm->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames == 0) return DVBS2_OK;
    if (int rc = demap_stage(h, syms, n_frames)) return rc;
    HCHK(hipMemcpyAsync(h->d_llr, ref_llr, (size_t)n_frames * h->dm->n_llr(), hipMemcpyHostToDevice, h->stream));
    if (h->dm->snr_device(h->d_syms, h->d_llr, n_frames, h->d_snr, h->stream)) return fail(DVBS2_EDEVICE, h->dm->error());
    HCHK(hipMemcpyAsync(snr_lin, h->d_snr, (size_t)n_frames * 4, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ chain */
struct dvbs2_chain {
    dvbs2_demap_t* dm = nullptr; // absent for an LLR-domain chain (dvbs2_chain_create_llr)
    dvbs2_ldpc_t* ldpc = nullptr; dvbs2_bch_t* bch = nullptr;
    int8_t* d_llr = nullptr; uint8_t* d_bits = nullptr; int32_t* d_corr = nullptr;
    int device = 0, max_frames = 0, n_llr = 0, ldpc_bytes = 0, msg_bytes = 0;
    // the call between enqueue and finish
    bool pending = false; int n_frames = 0; uint8_t* d_msg = nullptr; int32_t* d_bch_corr = nullptr; void* stream = nullptr;
    // host-pointer entries (dvbs2_chain_decode / dvbs2_chain_decode_llr): device copies of the caller's buffers, pinned landing buffers for
    // the outputs of a pageable caller and the streams in `pipe` (as dvbs2_ldpc_decode)
    float* hd_syms = nullptr; int8_t* hd_llr = nullptr; float* hd_n0 = nullptr; uint8_t* hd_msg = nullptr; int32_t* hd_ret = nullptr; int32_t* hd_corr = nullptr;
    HostPipe pipe;
    int host_chunk = 0; // DVBS2_HOST_CHUNK (experiments, tests), read once at create
};

static int chain_make(dvbs2_chain_t** h, int standard, int framesize, int rate, int constellation, bool with_demap,
                      int group_size, int max_frames, int device)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    dvbs2_chain* o = new (std::nothrow) dvbs2_chain();
    if (!o) return fail(DVBS2_EDEVICE, "out of memory");
    o->device = device; o->max_frames = max_frames;
    o->host_chunk = host_chunk_env();
    int rc = DVBS2_OK;
    if (with_demap) rc = dvbs2_demap_create(&o->dm, framesize, rate, constellation, max_frames, device);
    if (rc == DVBS2_OK) rc = dvbs2_ldpc_create(&o->ldpc, standard, framesize, rate, group_size, max_frames, device);
    if (rc == DVBS2_OK) rc = dvbs2_bch_create(&o->bch, standard, framesize, rate, max_frames, device);
    if (rc != DVBS2_OK) { std::string keep = g_err; dvbs2_chain_destroy(o); return fail(rc, keep); }
    o->n_llr = o->ldpc->dec->N();
    o->ldpc_bytes = o->ldpc->dec->out_bits_message() / 8;
    o->msg_bytes = o->bch->dec->code().k / 8;
    if ((o->dm && o->dm->dm->n_llr() != o->n_llr) || o->ldpc_bytes != o->bch->dec->code().n / 8) { dvbs2_chain_destroy(o); return fail(DVBS2_EINVAL, "inconsistent chain sizes"); }
    DeviceGuard guard(device);
    hipError_t e = guard.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess && o->dm) e = hipMalloc(&o->d_llr, (size_t)max_frames * o->n_llr);
    if (e == hipSuccess) e = hipMalloc(&o->d_bits, (size_t)max_frames * o->ldpc_bytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_corr, (size_t)max_frames * 4);
    if (e != hipSuccess) { dvbs2_chain_destroy(o); return fail(DVBS2_EDEVICE, hipGetErrorString(e)); }
    *h = o;
    return DVBS2_OK;
}

// LDPC (already enqueued) -> BCH on the same stream; the LDPC output never leaves HBM
// BCH straight from the LDPC decoder's state (hard decision + packing of ldpc_decoder_bb fused into the BCH kernel's load: no
// finalize launch, no packed-bit buffer in between)
static int chain_bch_range(dvbs2_chain_t* h, int frame_base, int n_frames, uint8_t* d_msg, int32_t* d_corr, hipStream_t stream)
{
    const int N = h->ldpc->dec->N();
    if (h->bch->dec->decode_device(nullptr, n_frames, d_msg, d_corr, stream, h->ldpc->dec->state() + (size_t)frame_base * N, N, frame_base))
        return fail(DVBS2_EDEVICE, h->bch->dec->error());
    return DVBS2_OK;
}
static int chain_bch(dvbs2_chain_t* h) { return chain_bch_range(h, 0, h->n_frames, h->d_msg, h->d_bch_corr, (hipStream_t)h->stream); }

// LDPC -> BCH on one stream; dm != nullptr: the LDPC sweep kernel demaps the symbols while it loads them
static int chain_enqueue_tail(dvbs2_chain_t* h, const int8_t* d_llr, const DemapFused* dm, int n_frames, int max_trials, uint8_t* d_msg,
                              int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    if (h->ldpc->dec->enqueue(d_llr, n_frames, max_trials, DVBS2_OM_MESSAGE, nullptr, nullptr, d_ldpc_ret, (hipStream_t)stream, 0, 0, dm))
        return fail(DVBS2_EDEVICE, h->ldpc->dec->error());
    h->pending = true; h->n_frames = n_frames; h->d_msg = d_msg; h->d_bch_corr = d_bch_corr ? d_bch_corr : h->d_corr; h->stream = stream;
    const int rc = chain_bch(h);
    if (rc != DVBS2_OK) { h->ldpc->dec->abort_all(); h->pending = false; } // nothing stays in flight or busy after a failed call
    return rc;
}

extern "C" {

int dvbs2_chain_set_descramble(dvbs2_chain_t* h, int enable)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    return dvbs2_bch_set_descramble(h->bch, enable);
}

void dvbs2_chain_destroy(dvbs2_chain_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    dvbs2_demap_destroy(h->dm); dvbs2_ldpc_destroy(h->ldpc); dvbs2_bch_destroy(h->bch);
    (void)hipFree(h->d_llr); (void)hipFree(h->d_bits); (void)hipFree(h->d_corr);
    (void)hipFree(h->hd_syms); (void)hipFree(h->hd_llr); (void)hipFree(h->hd_n0); (void)hipFree(h->hd_msg); (void)hipFree(h->hd_ret); (void)hipFree(h->hd_corr);
    host_pipe_destroy(h->pipe);
    delete h;
}

int dvbs2_chain_create(dvbs2_chain_t** h, int standard, int framesize, int rate, int constellation, int group_size, int max_frames, int device)
{
    API_TRY
    return chain_make(h, standard, framesize, rate, constellation, true, group_size, max_frames, device);
    API_CATCH
}

int dvbs2_chain_create_llr(dvbs2_chain_t** h, int standard, int framesize, int rate, int group_size, int max_frames, int device)
{
    API_TRY
    return chain_make(h, standard, framesize, rate, 0, false, group_size, max_frames, device);
    API_CATCH
}

int dvbs2_chain_params(const dvbs2_chain_t* h, int* n_syms, int* msg_bytes)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms) *n_syms = h->dm ? h->dm->dm->n_syms() : 0;
    if (msg_bytes) *msg_bytes = h->msg_bytes;
    return DVBS2_OK;
}

int dvbs2_chain_llr_params(const dvbs2_chain_t* h, int* n_llr, int* msg_bytes, int* group_size)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_llr) *n_llr = h->n_llr;
    if (msg_bytes) *msg_bytes = h->msg_bytes;
    if (group_size) *group_size = h->ldpc->dec->group_size();
    return DVBS2_OK;
}

int dvbs2_chain_enqueue_device(dvbs2_chain_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count,
                               int max_trials, uint8_t* d_msg, int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (!h->dm) return fail(DVBS2_EINVAL, "this chain starts at LLRs: use dvbs2_chain_enqueue_llr_device");
    if (h->pending) return fail(DVBS2_EINVAL, "previous call not finished");
    if (n_frames > h->max_frames) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && !d_msg)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames == 0) return DVBS2_OK;
    if (!d_syms || !d_n0 || (n0_count != 1 && n0_count != n_frames)) return fail(DVBS2_EINVAL, "bad argument");
    if (h->ldpc->dec->fused_demap_supported() && h->dm->dm->fusable()) { // symbols -> LDS inside the LDPC sweep kernel: no demapper launch, no LLR buffer
        const DemapFused dm = h->dm->dm->fused(d_syms, d_n0, n0_count);
        return chain_enqueue_tail(h, nullptr, &dm, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    }
    int rc = dvbs2_demap_soft_device(h->dm, d_syms, n_frames, d_n0, n0_count, h->d_llr, stream);
    if (rc == DVBS2_OK) rc = chain_enqueue_tail(h, h->d_llr, nullptr, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    return rc;
    API_CATCH
}

int dvbs2_chain_enqueue_llr_device(dvbs2_chain_t* h, const int8_t* d_llr, int n_frames, int max_trials, uint8_t* d_msg,
                                   int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->pending) return fail(DVBS2_EINVAL, "previous call not finished");
    if (n_frames > h->max_frames) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && (!d_llr || !d_msg))) return fail(DVBS2_EINVAL, "bad argument");
    if (((uintptr_t)d_llr) & 7u) return fail(DVBS2_EINVAL, "d_llr must be 8-byte aligned"); // (8-byte loads: include/dvbs2_fec_hip.h)
    if (n_frames == 0) return DVBS2_OK;
    return chain_enqueue_tail(h, d_llr, nullptr, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    API_CATCH
}

int dvbs2_chain_ldpc_profile(dvbs2_chain_t* h, int enable, double* total_ms, int* launches)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    return dvbs2_ldpc_profile(h->ldpc, enable, total_ms, launches);
}

const char* dvbs2_chain_ldpc_kernel_name(const dvbs2_chain_t* h) { return h ? h->ldpc->dec->kernel_name() : nullptr; }
int dvbs2_chain_ldpc_fallback_rounds(const dvbs2_chain_t* h) { return h ? h->ldpc->dec->fallback_rounds() : -1; }

int dvbs2_chain_finish(dvbs2_chain_t* h)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (!h->pending) return DVBS2_OK;
    h->pending = false;
    const int r = h->ldpc->dec->finish(0); // waits for the stream: demapper, LDPC and BCH of this call are done
    if (r < 0) return fail(DVBS2_EDEVICE, h->ldpc->dec->error());
    if (r > 0) { // the LDPC needed rounds beyond the enqueued ones and rewrote its output: run the BCH stage again
        int rc = chain_bch(h);
        if (rc != DVBS2_OK) return rc;
        HCHK(hipStreamSynchronize((hipStream_t)h->stream));
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_chain_decode_device(dvbs2_chain_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count,
                              int max_trials, uint8_t* d_msg, int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    int rc = dvbs2_chain_enqueue_device(h, d_syms, n_frames, d_n0, n0_count, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    if (rc != DVBS2_OK) { if (h) h->pending = false; return rc; }
    return dvbs2_chain_finish(h);
}

int dvbs2_chain_decode_llr_device(dvbs2_chain_t* h, const int8_t* d_llr, int n_frames, int max_trials, uint8_t* d_msg,
                                  int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    int rc = dvbs2_chain_enqueue_llr_device(h, d_llr, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    if (rc != DVBS2_OK) { if (h) h->pending = false; return rc; }
    return dvbs2_chain_finish(h);
}

} // extern "C"

// Host-pointer form of the fused chain (SURVEY 8(b) "dvbs2_fec_chain_decode(syms -> msg bytes)"): what the three blocks do with the
// item buffers GNU Radio hands them (lib/xfecframe_demapper_cb_impl.cc:101-186 -> lib/ldpc_decoder_bb_impl.cc:394-455 ->
// lib/bch_decoder_bb_impl.cc:84-117), as ONE call. The call is cut into chunks of whole LDPC groups and goes through host_pipe_run like
// dvbs2_ldpc_decode: chunk c runs on stream c mod kSlots in its own range of the LDPC state / message buffers and of the BCH syndrome words, its input
// copy (through one copy stream when the caller's buffer is page-locked) runs under the kernels of chunk c - 1 and its results go
// back while chunk c + 1 decodes. An 8PSK normal frame is 172.8 KB of symbols in and ~6 KB out: at the ~57 GB/s of the host link the
// chain is LINK-bound near 320 k frames/s -- below what the kernels do at a receiver's operating point (bench.py config3_host).
// in_syms: XFECFRAME symbols (a demapping chain) or null; in_llr: int8 LLRs (either kind of chain) or null.
static int chain_decode_host(dvbs2_chain_t* h, const float* in_syms, const int8_t* in_llr, int n_frames, const float* n0, int n0_count,
                             int max_trials, uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->pending) return fail(DVBS2_EINVAL, "previous call not finished");
    if (n_frames > h->max_frames) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && (!msg || (!in_syms && !in_llr)))) return fail(DVBS2_EINVAL, "bad argument");
    if (in_syms && !h->dm) return fail(DVBS2_EINVAL, "this chain starts at LLRs: use dvbs2_chain_decode_llr");
    if (in_syms && (!n0 || (n0_count != 1 && n0_count != n_frames))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    LdpcDecoderHip* dec = h->ldpc->dec;
    const size_t N = (size_t)dec->N(), mf = (size_t)h->max_frames, mb = (size_t)h->msg_bytes;
    const size_t ns = h->dm ? (size_t)h->dm->dm->n_syms() : 0;
    const int G = dec->group_size();
    const size_t ret_bytes = ((mf + G - 1) / G + kSlots) * 4;
    if (int rc = host_pipe_init(h->pipe)) return rc;
    const bool fused = in_syms && dec->fused_demap_supported() && h->dm->dm->fusable(); // symbols -> LDS inside the sweep kernel; else demapper launch -> LLR buffer
    if (in_syms && !h->hd_syms) HCHK(hipMalloc(&h->hd_syms, mf * ns * 8));
    if (in_syms && !h->hd_n0) HCHK(hipMalloc(&h->hd_n0, mf * 4));
    if ((in_llr || !fused) && !h->hd_llr) HCHK(hipMalloc(&h->hd_llr, mf * N));
    if (!h->hd_msg) HCHK(hipMalloc(&h->hd_msg, mf * mb));
    if (!h->hd_ret) HCHK(hipMalloc(&h->hd_ret, ret_bytes));
    if (!h->hd_corr) HCHK(hipMalloc(&h->hd_corr, mf * 4));
    HostCall call;
    if (int rc = host_add_output(h->pipe, call, n_frames, h->hd_msg, msg, mb, 1, mf * mb)) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, h->hd_ret, ldpc_ret, 4, G, ret_bytes)) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, h->hd_corr, bch_corr, 4, 1, mf * 4)) return rc;
    const void* in_ptr = in_syms ? (const void*)in_syms : (const void*)in_llr;
    const size_t in_frame_bytes = in_syms ? ns * 8 : N;
    const bool in_locked = host_range_page_locked(in_ptr, (size_t)n_frames * in_frame_bytes);
    call.plan = host_chunk_plan(n_frames, G, in_locked, in_syms != nullptr, h->host_chunk, "");
    call.use_copy_stream = in_locked;
    call.shared_input = in_syms && n0_count == 1;
    call.copy_in = [&](int c, int f0, int nf, hipStream_t cs) -> int {
        if (in_syms) {
            HCHK(hipMemcpyAsync(h->hd_syms + (size_t)f0 * ns * 2, in_syms + (size_t)f0 * ns * 2, (size_t)nf * ns * 8, hipMemcpyHostToDevice, cs));
            if (n0_count > 1) HCHK(hipMemcpyAsync(h->hd_n0 + f0, n0 + f0, (size_t)nf * 4, hipMemcpyHostToDevice, cs));
            else if (c == 0) HCHK(hipMemcpyAsync(h->hd_n0, n0, 4, hipMemcpyHostToDevice, cs));
        } else
            HCHK(hipMemcpyAsync(h->hd_llr + (size_t)f0 * N, in_llr + (size_t)f0 * N, (size_t)nf * N, hipMemcpyHostToDevice, cs));
        return DVBS2_OK;
    };
    call.enqueue = [&](int c, int f0, int nf, hipStream_t st) -> int {
        const float* dn0 = n0_count > 1 ? h->hd_n0 + f0 : h->hd_n0;
        const float* dsy = in_syms ? h->hd_syms + (size_t)f0 * ns * 2 : nullptr;
        int erc;
        if (fused) {
            const DemapFused dm = h->dm->dm->fused(dsy, dn0, n0_count > 1 ? nf : 1);
            erc = dec->enqueue(nullptr, nf, max_trials, DVBS2_OM_MESSAGE, nullptr, nullptr, h->hd_ret + f0 / G, st, c % kSlots, f0, &dm);
        } else {
            if (in_syms && h->dm->dm->soft_device(dsy, nf, dn0, n0_count > 1 ? nf : 1, h->hd_llr + (size_t)f0 * N, st)) return fail(DVBS2_EDEVICE, h->dm->dm->error());
            erc = dec->enqueue(h->hd_llr + (size_t)f0 * N, nf, max_trials, DVBS2_OM_MESSAGE, nullptr, nullptr, h->hd_ret + f0 / G, st, c % kSlots, f0, nullptr);
        }
        return erc ? fail(DVBS2_EDEVICE, dec->error()) : DVBS2_OK;
    };
    call.after_ldpc = [&](int f0, int nf, hipStream_t st) -> int { return chain_bch_range(h, f0, nf, h->hd_msg + (size_t)f0 * mb, h->hd_corr + f0, st); };
    return host_pipe_run(h->pipe, dec, call);
}

extern "C" {

int dvbs2_chain_decode(dvbs2_chain_t* h, const float* syms, int n_frames, const float* n0, int n0_count, int max_trials,
                       uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr)
{
    API_TRY
    if (n_frames > 0 && !syms) return fail(DVBS2_EINVAL, "bad argument");
    return chain_decode_host(h, syms, nullptr, n_frames, n0, n0_count, max_trials, msg, ldpc_ret, bch_corr);
    API_CATCH
}

int dvbs2_chain_decode_llr(dvbs2_chain_t* h, const int8_t* llr, int n_frames, int max_trials, uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr)
{
    API_TRY
    if (n_frames > 0 && !llr) return fail(DVBS2_EINVAL, "bad argument");
    return chain_decode_host(h, nullptr, llr, n_frames, nullptr, 0, max_trials, msg, ldpc_ret, bch_corr);
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ PLFRAME payload step */
struct dvbs2_plpayload {
    PlPayloadHip* pp = nullptr;
    float* d_in = nullptr; float* d_out = nullptr; float* d_par = nullptr; int32_t* d_cc = nullptr;
    hipStream_t stream = nullptr;
    int device = 0;
};

extern "C" {

int dvbs2_pl_scrambling_rn(int gold_code, uint8_t* rn, int n)
{
    API_TRY
    if (!rn || n < 0 || n > 360 * 90 + 22 * 36 || gold_code < 0 || gold_code >= (1 << 18) - 1) return fail(DVBS2_EINVAL, "bad argument");
    pl_scrambling_rn(gold_code, rn, n);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plpayload_create(dvbs2_plpayload_t** h, int gold_code, int n_slots, int has_pilots, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, false, [&](dvbs2_plpayload* o) { return o->pp = new (std::nothrow) PlPayloadHip(gold_code, n_slots, has_pilots, max_frames, device); });
    API_CATCH
}

void dvbs2_plpayload_destroy(dvbs2_plpayload_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_in); (void)hipFree(h->d_out); (void)hipFree(h->d_par); (void)hipFree(h->d_cc);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->pp;
    delete h;
}

int dvbs2_plpayload_params(const dvbs2_plpayload_t* h, int* payload_len, int* xfecframe_len, int* n_pilots)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (payload_len) *payload_len = h->pp->payload_len();
    if (xfecframe_len) *xfecframe_len = h->pp->xfecframe_len();
    if (n_pilots) *n_pilots = h->pp->n_pilots();
    return DVBS2_OK;
}

int dvbs2_plpayload_process_device(dvbs2_plpayload_t* h, const float* d_payload, int n_frames, const float* d_plheader_phase,
                                   const float* d_phase_inc, const int32_t* d_coarse_corrected, const float* d_pilot_phase,
                                   float* d_xfecframes, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!d_payload || !d_plheader_phase || !d_phase_inc || !d_coarse_corrected || !d_xfecframes ||
                                      (h->pp->n_pilots() > 0 && !d_pilot_phase)))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->pp->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->pp->process_device(d_payload, n_frames, d_plheader_phase, d_phase_inc, d_coarse_corrected, d_pilot_phase, d_xfecframes,
                              (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->pp->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plpayload_process(dvbs2_plpayload_t* h, const float* payload, int n_frames, const float* plheader_phase, const float* phase_inc,
                            const int32_t* coarse_corrected, const float* pilot_phase, float* xfecframes)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    const int np = h->pp->n_pilots();
    if (n_frames < 0 || (n_frames && (!payload || !plheader_phase || !phase_inc || !coarse_corrected || !xfecframes || (np > 0 && !pilot_phase))))
        return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->pp->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const size_t mf = h->pp->max_frames(), pl = h->pp->payload_len(), xl = h->pp->xfecframe_len(), nf = n_frames;
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_in) HCHK(hipMalloc(&h->d_in, mf * pl * 8));
    if (!h->d_out) HCHK(hipMalloc(&h->d_out, mf * xl * 8));
    if (!h->d_par) HCHK(hipMalloc(&h->d_par, mf * (2 + (np ? np : 1)) * 4));
    if (!h->d_cc) HCHK(hipMalloc(&h->d_cc, mf * 4));
    float* d_hph = h->d_par; float* d_inc = h->d_par + mf; float* d_pp = h->d_par + 2 * mf;
    HCHK(hipMemcpyAsync(h->d_in, payload, nf * pl * 8, hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(d_hph, plheader_phase, nf * 4, hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(d_inc, phase_inc, nf * 4, hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(h->d_cc, coarse_corrected, nf * 4, hipMemcpyHostToDevice, h->stream));
    if (np) HCHK(hipMemcpyAsync(d_pp, pilot_phase, nf * np * 4, hipMemcpyHostToDevice, h->stream));
    if (h->pp->process_device(h->d_in, n_frames, d_hph, d_inc, h->d_cc, d_pp, h->d_out, h->stream)) return fail(DVBS2_EDEVICE, h->pp->error());
    HCHK(hipMemcpyAsync(xfecframes, h->d_out, nf * xl * 8, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ PLFRAME front end: PLSC, phases, fine offset */
struct dvbs2_plframe {
    PlFrameHip* pf = nullptr;
    // staging of the host entries
    float* d_in = nullptr; float* d_out = nullptr; float* d_cf = nullptr; int32_t* d_cc = nullptr;
    float* d_est = nullptr; // sof | plheader | fine | pilot phases | fine_valid (int32) | plsc (uint8)
    hipStream_t stream = nullptr;
    int device = 0;
};

static int plframe_check(const dvbs2_plframe* h, const void* plframes, int n_frames, const void* cc, const void* cf)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!plframes || !cc))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames && h->pf->pls().n_pilots == 0 && !cf) return fail(DVBS2_EINVAL, "a pilotless handle needs coarse_foffset");
    if (n_frames > h->pf->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

static PlFrameEstimates plframe_est(const dvbs2_plframe_estimates_t* e)
{
    PlFrameEstimates o;
    if (e) { o.plsc_decoded = e->plsc_decoded; o.sof_phase = e->sof_phase; o.plheader_phase = e->plheader_phase;
             o.pilot_phase = e->pilot_phase; o.fine_foffset = e->fine_foffset; o.fine_valid = e->fine_valid; }
    return o;
}

// host entry: stage in, run, copy back what the caller asked for
static int plframe_host(dvbs2_plframe* h, const float* plframes, int n_frames, int trailing, const int32_t* cc, const float* cf,
                        float* xfecframes, const dvbs2_plframe_estimates_t* est)
{
    if (int rc = plframe_check(h, plframes, n_frames, cc, cf)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const PlsInfo& p = h->pf->pls();
    const size_t mf = h->pf->max_frames(), fl = p.plframe_len, xl = p.xfecframe_len, nf = n_frames, np = p.n_pilots;
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_in) HCHK(hipMalloc(&h->d_in, (mf * fl + 90) * 8));
    if (!h->d_out) HCHK(hipMalloc(&h->d_out, mf * xl * 8));
    if (!h->d_cf) HCHK(hipMalloc(&h->d_cf, mf * 4));
    if (!h->d_cc) HCHK(hipMalloc(&h->d_cc, mf * 4));
    if (!h->d_est) HCHK(hipMalloc(&h->d_est, mf * (4 + (np ? np : 1)) * 4 + mf));
    PlFrameEstimates d;
    d.sof_phase = h->d_est; d.plheader_phase = h->d_est + mf; d.fine_foffset = h->d_est + 2 * mf; d.pilot_phase = h->d_est + 3 * mf;
    d.fine_valid = reinterpret_cast<int32_t*>(h->d_est + (3 + (np ? np : 1)) * mf);
    d.plsc_decoded = reinterpret_cast<uint8_t*>(h->d_est + (4 + (np ? np : 1)) * mf);
    HCHK(hipMemcpyAsync(h->d_in, plframes, (nf * fl + (trailing ? 90 : 0)) * 8, hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(h->d_cc, cc, nf * 4, hipMemcpyHostToDevice, h->stream));
    if (cf) HCHK(hipMemcpyAsync(h->d_cf, cf, nf * 4, hipMemcpyHostToDevice, h->stream));
    if (h->pf->run_device(h->d_in, n_frames, trailing, h->d_cc, cf ? h->d_cf : nullptr, xfecframes ? h->d_out : nullptr, d, h->stream))
        return fail(DVBS2_EDEVICE, h->pf->error());
    if (xfecframes) HCHK(hipMemcpyAsync(xfecframes, h->d_out, nf * xl * 8, hipMemcpyDeviceToHost, h->stream));
    if (est) {
        if (est->sof_phase) HCHK(hipMemcpyAsync(est->sof_phase, d.sof_phase, nf * 4, hipMemcpyDeviceToHost, h->stream));
        if (est->plheader_phase) HCHK(hipMemcpyAsync(est->plheader_phase, d.plheader_phase, nf * 4, hipMemcpyDeviceToHost, h->stream));
        if (est->fine_foffset) HCHK(hipMemcpyAsync(est->fine_foffset, d.fine_foffset, nf * 4, hipMemcpyDeviceToHost, h->stream));
        if (est->pilot_phase && np) HCHK(hipMemcpyAsync(est->pilot_phase, d.pilot_phase, nf * np * 4, hipMemcpyDeviceToHost, h->stream));
        if (est->fine_valid) HCHK(hipMemcpyAsync(est->fine_valid, d.fine_valid, nf * 4, hipMemcpyDeviceToHost, h->stream));
        if (est->plsc_decoded) HCHK(hipMemcpyAsync(est->plsc_decoded, d.plsc_decoded, nf, hipMemcpyDeviceToHost, h->stream));
    }
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
}

extern "C" {

int dvbs2_plheader_symbols(int plsc, float* syms90)
{
    if (!syms90 || plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "bad argument");
    plheader_symbols(plsc, syms90);
    return DVBS2_OK;
}

int dvbs2_pls_parse(int plsc, int* plframe_len, int* payload_len, int* xfecframe_len, int* n_slots, int* n_pilots, int* n_mod)
{
    if (plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    const PlsInfo p = pls_parse(plsc);
    if (plframe_len) *plframe_len = p.plframe_len;
    if (payload_len) *payload_len = p.payload_len;
    if (xfecframe_len) *xfecframe_len = p.xfecframe_len;
    if (n_slots) *n_slots = p.n_slots;
    if (n_pilots) *n_pilots = p.n_pilots;
    if (n_mod) *n_mod = p.n_mod;
    return DVBS2_OK;
}

int dvbs2_plframe_create(dvbs2_plframe_t** h, int gold_code, int plsc, int max_frames, int device)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    // arguments first: a bad PLSC is the caller's mistake on any machine
    if (plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    { const PlsInfo p = pls_parse(plsc); if (p.n_mod == 0 && !p.dummy_frame) return fail(DVBS2_EINVAL, "plsc names a reserved MODCOD (29..31)"); }
    if (gold_code < 0 || gold_code >= (1 << 18) - 1) return fail(DVBS2_EINVAL, "gold code out of range");
    return make_handle(h, device, false, [&](dvbs2_plframe* o) { return o->pf = new (std::nothrow) PlFrameHip(gold_code, plsc, max_frames, device); });
    API_CATCH
}

void dvbs2_plframe_destroy(dvbs2_plframe_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_in); (void)hipFree(h->d_out); (void)hipFree(h->d_cf); (void)hipFree(h->d_cc); (void)hipFree(h->d_est);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->pf;
    delete h;
}

int dvbs2_plframe_params(const dvbs2_plframe_t* h, int* plframe_len, int* payload_len, int* xfecframe_len, int* n_slots, int* n_pilots,
                         int* n_mod)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    return dvbs2_pls_parse(h->pf->pls().plsc, plframe_len, payload_len, xfecframe_len, n_slots, n_pilots, n_mod);
}

int dvbs2_plframe_set_plsc_mode(dvbs2_plframe_t* h, int coherent, int soft)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    h->pf->set_plsc_mode(coherent, soft);
    return DVBS2_OK;
}

int dvbs2_plframe_set_expected_pls(dvbs2_plframe_t* h, const uint8_t* plsc_list, int n)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n < 0 || (n > 0 && !plsc_list)) return fail(DVBS2_EINVAL, "bad argument");
    if (int rc = h->pf->set_expected_pls(plsc_list, n)) return fail(rc == -1 ? DVBS2_EINVAL : DVBS2_EDEVICE, h->pf->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plframe_estimate_device(dvbs2_plframe_t* h, const float* d_plframes, int n_frames, int has_trailing_header,
                                  const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                                  const dvbs2_plframe_estimates_t* d_est, void* stream)
{
    API_TRY
    if (int rc = plframe_check(h, d_plframes, n_frames, d_coarse_corrected, d_coarse_foffset)) return rc;
    if (h->pf->run_device(d_plframes, n_frames, has_trailing_header, d_coarse_corrected, d_coarse_foffset, nullptr, plframe_est(d_est),
                          (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->pf->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plframe_process_device(dvbs2_plframe_t* h, const float* d_plframes, int n_frames, int has_trailing_header,
                                 const int32_t* d_coarse_corrected, const float* d_coarse_foffset, float* d_xfecframes,
                                 const dvbs2_plframe_estimates_t* d_est, void* stream)
{
    API_TRY
    if (int rc = plframe_check(h, d_plframes, n_frames, d_coarse_corrected, d_coarse_foffset)) return rc;
    if (n_frames && !d_xfecframes) return fail(DVBS2_EINVAL, "bad argument");
    if (h->pf->run_device(d_plframes, n_frames, has_trailing_header, d_coarse_corrected, d_coarse_foffset, d_xfecframes, plframe_est(d_est),
                          (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->pf->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plframe_estimate(dvbs2_plframe_t* h, const float* plframes, int n_frames, int has_trailing_header,
                           const int32_t* coarse_corrected, const float* coarse_foffset, const dvbs2_plframe_estimates_t* est)
{
    API_TRY
    return plframe_host(h, plframes, n_frames, has_trailing_header, coarse_corrected, coarse_foffset, nullptr, est);
    API_CATCH
}

int dvbs2_plframe_process(dvbs2_plframe_t* h, const float* plframes, int n_frames, int has_trailing_header,
                          const int32_t* coarse_corrected, const float* coarse_foffset, float* xfecframes,
                          const dvbs2_plframe_estimates_t* est)
{
    API_TRY
    if (n_frames > 0 && !xfecframes) return fail(DVBS2_EINVAL, "bad argument");
    return plframe_host(h, plframes, n_frames, has_trailing_header, coarse_corrected, coarse_foffset, xfecframes, est);
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ PLFRAME search: timing metric, lock state machine, gather */
struct dvbs2_plsync {
    PlSyncHip* ps = nullptr;
    float* d_in = nullptr; PlSyncFrame* d_frames = nullptr; // staging of the host entry
    hipStream_t stream = nullptr;
    int device = 0;
};
static_assert(sizeof(dvbs2_plsync_frame_t) == sizeof(PlSyncFrame) && offsetof(dvbs2_plsync_frame_t, metric) == offsetof(PlSyncFrame, metric) &&
              offsetof(dvbs2_plsync_frame_t, plsc) == offsetof(PlSyncFrame, plsc) && offsetof(dvbs2_plsync_frame_t, flags) == offsetof(PlSyncFrame, flags),
              "the public frame record is the kernel's");

extern "C" {

int dvbs2_plsync_taps(float* sof25, float* plsc32)
{
    if (!sof25 || !plsc32) return fail(DVBS2_EINVAL, "bad argument");
    plsync_taps(sof25, plsc32);
    return DVBS2_OK;
}

int dvbs2_plsync_thresholds(float* unlocked, float* locked)
{
    if (unlocked) *unlocked = kPlsyncThresholdUnlocked;
    if (locked) *locked = kPlsyncThresholdLocked;
    return DVBS2_OK;
}

int dvbs2_plsync_create(dvbs2_plsync_t** h, int plsc_or_minus1, int unlock_thresh, int max_symbols, int max_frames, int device)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return fail(DVBS2_EINVAL, "plsc out of range (-1 = decode every header, 0..127)");
    if (unlock_thresh < 1 || unlock_thresh > 255) return fail(DVBS2_EINVAL, "unlock_thresh out of range (1..255)");
    if (max_symbols < kPlsyncMinSymbols) return fail(DVBS2_EINVAL, "max_symbols must be at least 33282 + 90");
    if (max_frames < 1 || max_frames > (1 << 20)) return fail(DVBS2_EINVAL, "max_frames out of range (1..1048576)");
    return make_handle(h, device, false, [&](dvbs2_plsync* o) { return o->ps = new (std::nothrow) PlSyncHip(plsc_or_minus1, unlock_thresh, max_symbols, max_frames, device); });
    API_CATCH
}

void dvbs2_plsync_destroy(dvbs2_plsync_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_in); (void)hipFree(h->d_frames);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->ps;
    delete h;
}

int dvbs2_plsync_reset(dvbs2_plsync_t* h)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->ps->reset()) return fail(DVBS2_EDEVICE, h->ps->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_set_plsc_mode(dvbs2_plsync_t* h, int coherent, int soft)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    h->ps->set_plsc_mode(coherent, soft);
    return DVBS2_OK;
}

int dvbs2_plsync_set_expected_pls(dvbs2_plsync_t* h, const uint8_t* plsc_list, int n)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n < 0 || (n > 0 && !plsc_list)) return fail(DVBS2_EINVAL, "bad argument");
    if (int rc = h->ps->set_expected_pls(plsc_list, n)) return fail(rc == -1 ? DVBS2_EINVAL : DVBS2_EDEVICE, h->ps->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_metric_device(dvbs2_plsync_t* h, const float* d_syms, int n_syms, float* d_metric, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms < 0 || (n_syms && (!d_syms || !d_metric))) return fail(DVBS2_EINVAL, "bad argument");
    if (h->ps->metric_device(d_syms, n_syms, d_metric, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->ps->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_search_device(dvbs2_plsync_t* h, const float* d_syms, int n_syms, dvbs2_plsync_frame_t* d_frames, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms < 0 || !d_frames || (n_syms && !d_syms)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms > h->ps->max_symbols()) return fail(DVBS2_ESIZE, "n_syms exceeds max_symbols");
    if (h->ps->search_device(d_syms, n_syms, reinterpret_cast<PlSyncFrame*>(d_frames), (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->ps->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_finish(dvbs2_plsync_t* h, int* n_frames, int* consumed, int* state)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->ps->finish(n_frames, consumed, state)) return fail(DVBS2_EDEVICE, h->ps->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_search(dvbs2_plsync_t* h, const float* syms, int n_syms, dvbs2_plsync_frame_t* frames, int* n_frames, int* consumed, int* state)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms < 0 || !frames || (n_syms && !syms)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms > h->ps->max_symbols()) return fail(DVBS2_ESIZE, "n_syms exceeds max_symbols");
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_in) HCHK(hipMalloc(&h->d_in, (size_t)h->ps->max_symbols() * 8));
    if (!h->d_frames) HCHK(hipMalloc(&h->d_frames, (size_t)h->ps->max_frames() * sizeof(PlSyncFrame)));
    if (n_syms) HCHK(hipMemcpyAsync(h->d_in, syms, (size_t)n_syms * 8, hipMemcpyHostToDevice, h->stream));
    if (h->ps->search_device(h->d_in, n_syms, h->d_frames, h->stream)) return fail(DVBS2_EDEVICE, h->ps->error());
    int nf = 0;
    if (h->ps->finish(&nf, consumed, state)) return fail(DVBS2_EDEVICE, h->ps->error());
    if (nf) HCHK(hipMemcpy(frames, h->d_frames, (size_t)nf * sizeof(PlSyncFrame), hipMemcpyDeviceToHost));
    if (n_frames) *n_frames = nf;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_gather_device(dvbs2_plsync_t* h, const float* d_syms, const dvbs2_plsync_frame_t* d_frames, int n_frames, int wanted_plsc,
                               float* d_plframes, int32_t* d_count, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (wanted_plsc < 0 || wanted_plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    if (n_frames < 0 || !d_count || (n_frames && (!d_syms || !d_frames || !d_plframes))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->ps->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->ps->gather_device(d_syms, reinterpret_cast<const PlSyncFrame*>(d_frames), n_frames, wanted_plsc, d_plframes, d_count, (hipStream_t)stream))
        return fail(DVBS2_EDEVICE, h->ps->error());
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ coarse frequency offset estimate */
struct dvbs2_plcoarse {
    PlCoarseHip* pc = nullptr;
    float* d_hdr = nullptr; uint8_t* d_plsc = nullptr; float* d_out = nullptr; // staging of the host entry
    hipStream_t stream = nullptr;
    int device = 0;
};

static int plcoarse_check(const dvbs2_plcoarse* h, const void* src, int n_frames)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && !src)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->pc->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

static PlCoarseOut plcoarse_out(float* foffset, int32_t* corrected, int32_t* new_est)
{
    PlCoarseOut o;
    o.foffset = foffset; o.corrected = corrected; o.new_est = new_est;
    return o;
}

extern "C" {

int dvbs2_plcoarse_weights(int full, float* w)
{
    if (!w) return fail(DVBS2_EINVAL, "bad argument");
    return plcoarse_weights(full, w);
}

int dvbs2_plcoarse_create(dvbs2_plcoarse_t** h, int period, int plsc_or_minus1, int max_frames, int device)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (period < 1) return fail(DVBS2_EINVAL, "period must be at least 1");
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return fail(DVBS2_EINVAL, "plsc out of range (-1 = not known, 0..127)");
    if (max_frames < 1 || max_frames > (1 << 20)) return fail(DVBS2_EINVAL, "max_frames out of range (1..1048576)");
    return make_handle(h, device, false, [&](dvbs2_plcoarse* o) { return o->pc = new (std::nothrow) PlCoarseHip(period, plsc_or_minus1, max_frames, device); });
    API_CATCH
}

void dvbs2_plcoarse_destroy(dvbs2_plcoarse_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_hdr); (void)hipFree(h->d_plsc); (void)hipFree(h->d_out);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->pc;
    delete h;
}

int dvbs2_plcoarse_reset(dvbs2_plcoarse_t* h)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->pc->reset()) return fail(DVBS2_EDEVICE, h->pc->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plcoarse_estimate_device(dvbs2_plcoarse_t* h, const float* d_plframes, int64_t stride_syms, const uint8_t* d_plsc, int n_frames,
                                   float* d_coarse_foffset, int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream)
{
    API_TRY
    if (int rc = plcoarse_check(h, d_plframes, n_frames)) return rc;
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!d_plsc && h->pc->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array");
    if (h->pc->frames_device(d_plframes, stride_syms, d_plsc, n_frames, plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est),
                             (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->pc->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plcoarse_estimate_records_device(dvbs2_plcoarse_t* h, const float* d_syms, int n_syms, int64_t base_index,
                                           const dvbs2_plsync_frame_t* d_frames, int n_frames, float* d_coarse_foffset,
                                           int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream)
{
    API_TRY
    if (int rc = plcoarse_check(h, d_frames, n_frames)) return rc;
    if (n_syms < 0 || (n_frames && !d_syms)) return fail(DVBS2_EINVAL, "bad argument");
    if (h->pc->records_device(d_syms, n_syms, reinterpret_cast<const PlSyncFrame*>(d_frames), n_frames, base_index,
                              plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est), (hipStream_t)stream))
        return fail(DVBS2_EDEVICE, h->pc->error());
    return DVBS2_OK;
    API_CATCH
}

// host entry: stage the 90 header symbols of every frame, run, copy back what the caller asked for
int dvbs2_plcoarse_estimate(dvbs2_plcoarse_t* h, const float* plframes, int64_t stride_syms, const uint8_t* plsc, int n_frames,
                            float* coarse_foffset, int32_t* coarse_corrected, int32_t* new_est)
{
    API_TRY
    if (int rc = plcoarse_check(h, plframes, n_frames)) return rc;
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!plsc && h->pc->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array");
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const size_t mf = h->pc->max_frames(), nf = n_frames;
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_hdr) HCHK(hipMalloc(&h->d_hdr, mf * 90 * 8));
    if (!h->d_plsc) HCHK(hipMalloc(&h->d_plsc, mf));
    if (!h->d_out) HCHK(hipMalloc(&h->d_out, mf * 3 * 4));
    HCHK(hipMemcpy2DAsync(h->d_hdr, 90 * 8, plframes, (size_t)stride_syms * 8, 90 * 8, nf, hipMemcpyHostToDevice, h->stream));
    if (plsc) HCHK(hipMemcpyAsync(h->d_plsc, plsc, nf, hipMemcpyHostToDevice, h->stream));
    float* d_fo = h->d_out; int32_t* d_cc = reinterpret_cast<int32_t*>(h->d_out + mf); int32_t* d_ne = reinterpret_cast<int32_t*>(h->d_out + 2 * mf);
    if (h->pc->frames_device(h->d_hdr, 90, plsc ? h->d_plsc : nullptr, n_frames, plcoarse_out(d_fo, d_cc, d_ne), h->stream))
        return fail(DVBS2_EDEVICE, h->pc->error());
    if (coarse_foffset) HCHK(hipMemcpyAsync(coarse_foffset, d_fo, nf * 4, hipMemcpyDeviceToHost, h->stream));
    if (coarse_corrected) HCHK(hipMemcpyAsync(coarse_corrected, d_cc, nf * 4, hipMemcpyDeviceToHost, h->stream));
    if (new_est) HCHK(hipMemcpyAsync(new_est, d_ne, nf * 4, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ rotator */
struct dvbs2_rotator {
    RotatorHip* rot = nullptr;
    float* d_buf = nullptr; size_t cap = 0; // staging of the host entry, grown on demand
    hipStream_t stream = nullptr;
    int device = 0;
};

extern "C" {

int dvbs2_rotator_create(dvbs2_rotator_t** h, double phase_inc, int device)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    if (!(phase_inc == phase_inc) || phase_inc - phase_inc != 0.0) return fail(DVBS2_EINVAL, "phase_inc must be finite");
    return make_handle(h, device, false, [&](dvbs2_rotator* o) { return o->rot = new (std::nothrow) RotatorHip(phase_inc, device); });
    API_CATCH
}

void dvbs2_rotator_destroy(dvbs2_rotator_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_buf);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->rot;
    delete h;
}

int dvbs2_rotator_reset(dvbs2_rotator_t* h)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    h->rot->reset();
    return DVBS2_OK;
}

int dvbs2_rotator_set_phase_inc(dvbs2_rotator_t* h, double phase_inc)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->rot->set_phase_inc(phase_inc)) return fail(DVBS2_EINVAL, h->rot->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_schedule(dvbs2_rotator_t* h, int64_t offset, double phase_inc)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->rot->schedule(offset, phase_inc)) return fail(DVBS2_EINVAL, h->rot->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_seek(dvbs2_rotator_t* h, int64_t n_syms)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->rot->seek(n_syms)) return fail(DVBS2_EINVAL, h->rot->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_position(const dvbs2_rotator_t* h, int64_t* n_syms, int* queued)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms) *n_syms = h->rot->position();
    if (queued) *queued = h->rot->queued();
    return DVBS2_OK;
}

int dvbs2_rotator_rotate_device(dvbs2_rotator_t* h, const float* d_in, int n_syms, float* d_out, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms < 0 || (n_syms && (!d_in || !d_out))) return fail(DVBS2_EINVAL, "bad argument");
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) return fail(DVBS2_EINVAL, "symbol buffers must be 8-byte aligned");
    if (h->rot->rotate_device(d_in, n_syms, d_out, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->rot->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_measure(int device, int n_syms, int regions, double* rotate_ms, double* copy_ms)
{
    API_TRY
    if (!rotate_ms || !copy_ms) return fail(DVBS2_EINVAL, "bad argument");
    if (int rc = check_device(device)) return rc;
    std::string err;
    if (rotator_measure(device, n_syms, regions, rotate_ms, copy_ms, &err)) return fail(err == "bad argument" ? DVBS2_EINVAL : DVBS2_EDEVICE, err);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_rotate(dvbs2_rotator_t* h, const float* in, int n_syms, float* out)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_syms < 0 || (n_syms && (!in || !out))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const size_t bytes = (size_t)n_syms * 8;
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (h->cap < bytes) {
        (void)hipFree(h->d_buf); h->d_buf = nullptr; h->cap = 0;
        HCHK(hipMalloc(&h->d_buf, bytes));
        h->cap = bytes;
    }
    HCHK(hipMemcpyAsync(h->d_buf, in, bytes, hipMemcpyHostToDevice, h->stream));
    if (h->rot->rotate_device(h->d_buf, n_syms, h->d_buf, h->stream)) return fail(DVBS2_EDEVICE, h->rot->error());
    HCHK(hipMemcpyAsync(out, h->d_buf, bytes, hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ symbol timing recovery */
struct dvbs2_symsync {
    SymSyncHip* ss = nullptr;
    float* d_in = nullptr; float* d_out = nullptr; int64_t* d_idx = nullptr; double* d_mu = nullptr; // staging of the host entry
    size_t in_cap = 0, out_cap = 0;
    hipStream_t stream = nullptr;
    int device = 0;
};

static int symsync_make(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp_method,
                        const float* bank, int max_streams, int max_samples, int device)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = SymSyncHip::check_args(sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, false, [&](dvbs2_symsync* o) {
        return o->ss = new (std::nothrow) SymSyncHip(sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, bank, max_streams, max_samples, device);
    });
}

extern "C" {

int dvbs2_symsync_loop_constants(int sps, float loop_bw, float damping, float rolloff, float* Kp, float* K1, float* K2)
{
    if (sps < 2 || (sps & 1)) return fail(DVBS2_EINVAL, "sps has to be an even integer >= 2");
    symsync_loop_constants(sps, loop_bw, damping, rolloff, Kp, K1, K2);
    return DVBS2_OK;
}

int dvbs2_symsync_geometry(int sps, int rrc_delay, int n_subfilt, int interp_method, int* subfilt_len, int* subfilt_delay, int* history)
{
    if (symsync_geometry(sps, rrc_delay, n_subfilt, interp_method, subfilt_len, subfilt_delay, history)) return fail(DVBS2_EINVAL, "bad argument");
    return DVBS2_OK;
}

int dvbs2_symsync_taps(int sps, float rolloff, int rrc_delay, int n_subfilt, float* bank)
{
    API_TRY
    if (symsync_taps(sps, rolloff, rrc_delay, n_subfilt, bank)) return fail(DVBS2_EINVAL, "bad argument");
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_symsync_create(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp_method,
                         int max_streams, int max_samples, int device)
{
    API_TRY
    return symsync_make(h, sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, nullptr, max_streams, max_samples, device);
    API_CATCH
}

int dvbs2_symsync_create_taps(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt,
                              int interp_method, const float* bank, int max_streams, int max_samples, int device)
{
    API_TRY
    if (h) *h = nullptr;
    if (!bank) return fail(DVBS2_EINVAL, "null bank");
    return symsync_make(h, sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, bank, max_streams, max_samples, device);
    API_CATCH
}

void dvbs2_symsync_destroy(dvbs2_symsync_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_in); (void)hipFree(h->d_out); (void)hipFree(h->d_idx); (void)hipFree(h->d_mu);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->ss;
    delete h;
}

int dvbs2_symsync_reset(dvbs2_symsync_t* h)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->ss->reset()) return fail(DVBS2_EDEVICE, h->ss->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_symsync_params(const dvbs2_symsync_t* h, int* subfilt_len, int* subfilt_delay, int* history, float* Kp, float* K1, float* K2)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    const SymSyncGeom& g = h->ss->geom();
    if (subfilt_len) *subfilt_len = g.subfilt_len;
    if (subfilt_delay) *subfilt_delay = g.subfilt_delay;
    if (history) *history = g.history;
    if (Kp) *Kp = h->ss->Kp();
    if (K1) *K1 = g.K1;
    if (K2) *K2 = g.K2;
    return DVBS2_OK;
}

int dvbs2_symsync_work_device(dvbs2_symsync_t* h, const float* d_in, int64_t in_stride, const int* n_in, int n_streams, float* d_out,
                              int64_t out_stride, int max_out, int64_t* d_strobe_idx, double* d_mu, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_streams < 1 || !n_in || !d_in || max_out < 0 || (max_out && !d_out)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_streams > h->ss->max_streams()) return fail(DVBS2_ESIZE, "n_streams exceeds max_streams");
    if (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_strobe_idx | (uintptr_t)d_mu) & 7) return fail(DVBS2_EINVAL, "buffers must be 8-byte aligned");
    int most = 0;
    for (int s = 0; s < n_streams; s++) {
        if (n_in[s] < 0) return fail(DVBS2_EINVAL, "negative sample count");
        if (n_in[s] > h->ss->max_samples()) return fail(DVBS2_ESIZE, "n_in exceeds max_samples");
        most = std::max(most, n_in[s]);
    }
    if (n_streams > 1 && (in_stride < most || out_stride < max_out)) return fail(DVBS2_EINVAL, "a stride below the length of a stream");
    if (h->ss->work_device(reinterpret_cast<const float2*>(d_in), in_stride, n_in, n_streams, reinterpret_cast<float2*>(d_out), out_stride, max_out,
                           d_strobe_idx, d_mu, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->ss->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_symsync_finish(dvbs2_symsync_t* h, int* n_out, int* consumed, int* status)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->ss->finish(n_out, consumed, status) < 0) return fail(DVBS2_EDEVICE, h->ss->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_symsync_state(dvbs2_symsync_t* h, int stream_index, dvbs2_symsync_state_t* out)
{
    API_TRY
    if (!h || !out) return fail(DVBS2_EINVAL, "bad argument");
    if (stream_index < 0 || stream_index >= h->ss->max_streams()) return fail(DVBS2_EINVAL, "stream index out of range");
    SymSyncState s;
    if (h->ss->state(stream_index, &s)) return fail(DVBS2_EDEVICE, h->ss->error());
    out->vi = s.vi; out->cnt = s.cnt; out->mu = s.mu; out->n_read = s.n_read; out->last_xi_re = s.last_xi.x; out->last_xi_im = s.last_xi.y;
    out->jump = s.jump; out->init = s.init; out->status = s.status; out->reserved = 0;
    return DVBS2_OK;
    API_CATCH
}

// host entry, stream 0 of the handle: stage, run, copy back what the caller asked for
int dvbs2_symsync_work(dvbs2_symsync_t* h, const float* in, int n_in, float* out, int max_out, int64_t* strobe_idx, double* mu, int* n_out,
                       int* consumed, int* status)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_in < 0 || max_out < 0 || (n_in && !in) || (max_out && !out)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_in > h->ss->max_samples()) return fail(DVBS2_ESIZE, "n_in exceeds max_samples");
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    const size_t ni = std::max(n_in, 1), no = std::max(max_out, 1);
    if (h->in_cap < ni) {
        (void)hipFree(h->d_in); h->d_in = nullptr; h->in_cap = 0;
        HCHK(hipMalloc(&h->d_in, ni * 8));
        h->in_cap = ni;
    }
    if (h->out_cap < no) {
        (void)hipFree(h->d_out); (void)hipFree(h->d_idx); (void)hipFree(h->d_mu);
        h->d_out = nullptr; h->d_idx = nullptr; h->d_mu = nullptr; h->out_cap = 0;
        HCHK(hipMalloc(&h->d_out, no * 8)); HCHK(hipMalloc(&h->d_idx, no * 8)); HCHK(hipMalloc(&h->d_mu, no * 8));
        h->out_cap = no;
    }
    if (n_in) HCHK(hipMemcpyAsync(h->d_in, in, (size_t)n_in * 8, hipMemcpyHostToDevice, h->stream));
    if (h->ss->work_device(reinterpret_cast<const float2*>(h->d_in), n_in, &n_in, 1, reinterpret_cast<float2*>(h->d_out), max_out, max_out,
                           h->d_idx, h->d_mu, h->stream)) return fail(DVBS2_EDEVICE, h->ss->error());
    int k = 0, c = 0, st = 0;
    if (h->ss->finish(&k, &c, &st) < 0) return fail(DVBS2_EDEVICE, h->ss->error());
    if (k) {
        HCHK(hipMemcpy(out, h->d_out, (size_t)k * 8, hipMemcpyDeviceToHost));
        if (strobe_idx) HCHK(hipMemcpy(strobe_idx, h->d_idx, (size_t)k * 8, hipMemcpyDeviceToHost));
        if (mu) HCHK(hipMemcpy(mu, h->d_mu, (size_t)k * 8, hipMemcpyDeviceToHost));
    }
    if (n_out) *n_out = k;
    if (consumed) *consumed = c;
    if (status) *status = st;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ BBFRAME de-header */
struct dvbs2_bbdeheader {
    BbDeheaderHip* bb = nullptr;
    uint8_t* d_in = nullptr; uint8_t* d_out = nullptr; // staging of the host entry
    hipStream_t stream = nullptr;
    int device = 0;
};

extern "C" {

int dvbs2_bbdeheader_create_raw(dvbs2_bbdeheader_t** h, int kbch_bits, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, false, [&](dvbs2_bbdeheader* o) { return o->bb = new (std::nothrow) BbDeheaderHip(kbch_bits, max_frames, device); });
    API_CATCH
}

int dvbs2_bbdeheader_create(dvbs2_bbdeheader_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle pointer");
    *h = nullptr;
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return dvbs2_bbdeheader_create_raw(h, (int)fi.bch_k, max_frames, device); // d_kbch_bytes, d_max_dfl (:58-61)
    API_CATCH
}

void dvbs2_bbdeheader_destroy(dvbs2_bbdeheader_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipFree(h->d_in); (void)hipFree(h->d_out);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h->bb;
    delete h;
}

int dvbs2_bbdeheader_params(const dvbs2_bbdeheader_t* h, int* kbch_bytes, int* max_dfl_bits, int* max_out_bytes_per_frame)
{
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (kbch_bytes) *kbch_bytes = h->bb->kbch_bytes();
    if (max_dfl_bits) *max_dfl_bits = h->bb->max_dfl();
    if (max_out_bytes_per_frame) *max_out_bytes_per_frame = h->bb->max_out_bytes_per_frame();
    return DVBS2_OK;
}

int dvbs2_bbdeheader_process_device(dvbs2_bbdeheader_t* h, const uint8_t* d_bbframes, int n_frames, uint8_t* d_ts_out, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!d_bbframes || !d_ts_out))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->bb->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (h->bb->process_device(d_bbframes, n_frames, d_ts_out, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->bb->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_finish(dvbs2_bbdeheader_t* h, int64_t* produced, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    BbdhState st;
    if (h->bb->state(&st, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->bb->error());
    if (produced) *produced = (int64_t)st.produced;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_counters(dvbs2_bbdeheader_t* h, dvbs2_bbdeheader_counters_t* out, void* stream)
{
    API_TRY
    if (!h || !out) return fail(DVBS2_EINVAL, "bad argument");
    BbdhState st;
    if (h->bb->state(&st, (hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->bb->error());
    out->packets = st.packets; out->errors = st.errors; out->bbframes = st.bbframes; out->dropped = st.dropped; out->gaps = st.gaps;
    out->overruns = st.overruns; out->synched = st.synched; out->partial_ts_bytes = st.partial;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_reset(dvbs2_bbdeheader_t* h, void* stream)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (h->bb->reset((hipStream_t)stream)) return fail(DVBS2_EDEVICE, h->bb->error());
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_process(dvbs2_bbdeheader_t* h, const uint8_t* bbframes, int n_frames, uint8_t* ts_out, int64_t* produced)
{
    API_TRY
    if (!h) return fail(DVBS2_EINVAL, "null handle");
    if (n_frames < 0 || (n_frames && (!bbframes || !ts_out))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->bb->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (produced) *produced = 0;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const size_t mf = h->bb->max_frames(), fb = h->bb->kbch_bytes(), ob = h->bb->max_out_bytes_per_frame();
    if (!h->stream) HCHK(hipStreamCreate(&h->stream));
    if (!h->d_in) HCHK(hipMalloc(&h->d_in, mf * fb));
    if (!h->d_out) HCHK(hipMalloc(&h->d_out, mf * ob));
    if (n_frames) HCHK(hipMemcpyAsync(h->d_in, bbframes, (size_t)n_frames * fb, hipMemcpyHostToDevice, h->stream));
    if (h->bb->process_device(h->d_in, n_frames, h->d_out, h->stream)) return fail(DVBS2_EDEVICE, h->bb->error());
    BbdhState st;
    if (h->bb->state(&st, h->stream)) return fail(DVBS2_EDEVICE, h->bb->error());
    if (st.produced > 0) {
        HCHK(hipMemcpyAsync(ts_out, h->d_out, (size_t)st.produced, hipMemcpyDeviceToHost, h->stream));
        HCHK(hipStreamSynchronize(h->stream));
    }
    if (produced) *produced = (int64_t)st.produced;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
