// host_pipe.h -- the chunked host pipeline behind the host-buffer entries that end in the LDPC decoder (dvbs2_ldpc_decode,
// dvbs2_chain_decode[_llr]). Internal, not installed.
#pragma once
#include <functional>
#include <utility>
#include <vector>
#include "c_api_common.h"
#include "ldpc_hip.h"

namespace dvbs2 {

// Is [p, p + bytes) ONE page-locked host range the copy engine can address (hipHostMalloc'ed, or registered with dvbs2_host_register /
// hipHostRegister)? Decided from the runtime's own record of the allocation that holds p -- its start and size
// (HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR / RANGE_SIZE) must cover the last byte -- so two registrations with a pageable hole between
// them are not mistaken for one. When the runtime cannot answer, the range counts as pageable: the call then stages through the
// handle's own pinned buffers, which is always correct.
bool host_range_page_locked(const void* p, size_t bytes);

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

int host_pipe_init(HostPipe& p);
void host_pipe_destroy(HostPipe& p); // (under the handle's DeviceGuard)

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
int host_add_output(HostPipe& p, HostCall& call, int n_frames, const void* dev, void* user, size_t unit_bytes, int frames_per_unit, size_t pinned_bytes);

// The pipeline: chunk c of the plan uses slot and stream c % kSlots (its own range of the decoder's state and message buffers); its input
// copy runs under the kernels of chunk c - 1 and its results go back while chunk c + 1 decodes.
int host_pipe_run(HostPipe& p, LdpcDecoderHip* dec, const HostCall& call);

} // namespace dvbs2
