// symsync_hip.h -- symbol timing recovery on the device: symbol_sync_cc_impl::loop (reference lib/symbol_sync_cc_impl.cc:283-401)
// with its four interpolators (:23-66, :122-132), its loop constants (:156-199), its state kept across calls and the strobe
// indices the block uses to move tags (:446-488). The polyphase interpolator is also the matched filter (an RRC filter bank).
//
// The loop is a feedback loop: the error at strobe k sets mu, the subfilter and the basepoint of strobe k + 1, so one stream
// cannot be cut across time. ONE WAVEFRONT PER STREAM (a 64-thread workgroup, grid = streams):
//   lanes 0..31   the output interpolant (basepoint m_k), lanes 32..63 the zero-crossing interpolant (basepoint m_k - sps / 2)
//   polyphase     lane j of a half takes taps j, j + 32, j + 64, ... of the subfilter in ascending order (float, no contraction),
//                 then a xor butterfly 16, 8, 4, 2, 1 inside the half leaves the same bits in every lane of the half
//   Farrow        linear / quadratic / cubic are four-tap scalar expressions, evaluated by every lane of the half in the
//                 reference's own order of operations
//   error         e = zc.re (last.re - out.re) + zc.im (last.im - out.im) in float after one exchange between the halves
//   PI + counter  uniform IEEE double, as the reference: vp = (double)(K1 e), vi += (double)(K2 e), W1, W2,
//                 floor((cnt - W1) / W2) + 2, mu by a true division
// LDS: the subfilter bank as [subfilter][tap] (polyphase only) and a ring of kSymsyncRing samples. The wavefront holds the next
// kSymsyncChunk samples in registers -- their global loads are issued before the current chunk is walked -- and moves them into
// the ring when a strobe first reaches past what the ring holds.
//
// Defined where the reference only asserts: floor(n_subfilt mu) is clamped to [0, n_subfilt - 1]; a stream stops at the strobe
// where W1 or W2 is not positive (status 1), where W1 or W2 is NaN (status 2), or where the next jump is not in [1, 2^30]
// (status 3); a stopped stream reports the n_out and consumed it reached and returns at once in later calls until reset. A
// stream that has not started consumes nothing from a call that presents fewer than 2 samples (the reference would report 2
// consumed samples whatever it was given). Every iteration advances by at least one sample, so the walk terminates.
//
// The RRC prototype of symsync_taps is designed here from the closed-form impulse response: firdes::root_raised_cosine belongs
// to GNU Radio and is not available to compare with, so the bank is UNPINNED against it (create_taps takes firdes's own taps).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kSymsyncRing = 1024;      // samples in the LDS ring (a power of two)
constexpr int kSymsyncChunk = 256;      // samples held in registers ahead of the ring: 4 per lane
constexpr int kSymsyncMaxLds = 65536;   // ring + bank
constexpr int kSymsyncMaxJump = 1 << 30;

struct SymSyncState { // per stream, lives on the device
    double vi, cnt, mu;
    int64_t n_read;   // samples consumed since create / reset
    float2 last_xi;
    int32_t jump, init, status, parity; // parity: which of the two history buffers holds the history
};

struct SymSyncResult { int32_t n_out, consumed, status, reserved; }; // of the last call, per stream

struct SymSyncGeom {
    int32_t sps, interp, n_subfilt, subfilt_len, subfilt_delay, history;
    float K1, K2;
};

// set_gted_gain and set_pi_constants (:156-199) with the reference's float / double mix
void symsync_loop_constants(int sps, float loop_bw, float damping, float rolloff, float* Kp, float* K1, float* K2);
// subfilter length and delay (:68-80) and the block's history (:244-256); -1 on a bad argument
int symsync_geometry(int sps, int rrc_delay, int n_subfilt, int interp, int* subfilt_len, int* subfilt_delay, int* history);
// n_subfilt * subfilt_len floats, [subfilter][tap], each subfilter flipped (:82-110); -1 on a bad argument
int symsync_taps(int sps, float rolloff, int rrc_delay, int n_subfilt, float* bank);

class SymSyncHip : public StreamStage {
public:
    // bank: n_subfilt * subfilt_len floats as symsync_taps lays them out, or null to design them here
    SymSyncHip(int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp, const float* bank,
               int max_streams, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp, int max_streams,
                                  int max_samples);
    const SymSyncGeom& geom() const { return g_; }
    float Kp() const { return Kp_; }
    int reset();
    // DEVICE pointers except n_in (host, one count per stream). Stream s reads d_in + s * in_stride samples and writes
    // d_out / d_strobe_idx / d_mu + s * out_stride, at most max_out of each
    int work_device(const float2* d_in, int64_t in_stride, const int* n_in, int n_streams, float2* d_out, int64_t out_stride, int max_out,
                    int64_t* d_strobe_idx, double* d_mu, hipStream_t stream);
    // One call in flight per handle: the sample counts and the results of a call live in one buffer each, so a second
    // work_device on ANOTHER stream needs a finish() first; calls on the same stream may follow each other (finish then reports the last)
    // waits for the last work_device; each array nullable, n_streams entries of the last call
    int finish(int* n_out, int* consumed, int* status);
    int state(int s, SymSyncState* out);

private:
    SymSyncGeom g_{};
    float Kp_ = 0.0f;
    int last_streams_ = 0;
    hipStream_t last_stream_ = nullptr;
    float* d_bank_ = nullptr;
    float2* d_hist_ = nullptr;         // max_streams * 2 * history
    SymSyncState* d_state_ = nullptr;
    SymSyncResult* d_res_ = nullptr;
    int* d_nin_ = nullptr;
    std::vector<SymSyncResult> res_;
};

} // namespace dvbs2
