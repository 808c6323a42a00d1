// pulse_hip.h -- pulse shaping on the device, the step behind the PL framer (plframer_hip.h): an integer-factor interpolating FIR with
// real taps over complex symbols, on a batch of independent streams whose histories stay on the device between calls. In the
// reference's transmit flowgraph (apps/dvbs2-tx:638-686) this is GNU Radio's interp_fir_filter_ccf over firdes.root_raised_cosine taps,
// optionally scaled by scale_rrc_taps (apps/dvbs2-tx:39-81); neither block is in the reference tree, so the stage is UNPINNED against
// them. What is pinned is the arithmetic, which tests/pulse_model.py restates and the device equals bit for bit:
//   y[m sps + p] = sum over k = 0, 1, ... while p + k sps < ntaps of h[p + k sps] * x[m - k]
//   real and imaginary part apart, each term a float product and then a float addition (no contraction), in ascending k, onto an
//   accumulator that starts at +0.0f; x[j] for j < 0 is the stream's history, zeros after create / reset.
// n_syms symbols in give n_syms sps samples out; the signal is delayed by (ntaps - 1) / 2 samples and nothing is dropped.
//
// Kernel: grid.y the stream, grid.x tiles of kPulseTile symbols. A block stages its tile and the `history` symbols before it in LDS once
// (symbols before the call come from the stream's history buffer): one HBM read per symbol plus the halo. A thread owns PAIRS of
// consecutive output samples (sps is even: a pair lies in one symbol), consecutive lanes consecutive pairs, so a wavefront stores 1 KiB in
// a row -- 16 bytes per lane where the output is 16-byte aligned, two 8-byte stores where it is not, the same bits. At sps 2 every pair
// has phase 0 and all lanes use the same taps: they are read through scalar loads; for sps > 2 the taps sit in LDS behind the symbols.
// The history of the next call -- the last `history` symbols of old history then input -- is written by a second, tiny launch behind
// the first (one block per stream, read, barrier, write), so no block of the first can see it change.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kPulseTile = 512;     // symbols per block
constexpr int kPulseMaxTerms = 129; // ceil(ntaps / sps) at most: history <= 128 symbols, one block of the history launch

// Host only. ntaps = 2 sps rrc_delay + 1, history = ceil(ntaps / sps) - 1 symbols, delay = sps rrc_delay samples; each nullable.
// -1: sps is not an even integer in 2..64 or rrc_delay not in 1..64 (the bounds of symsync_geometry)
int pulse_geometry(int sps, int rrc_delay, int* ntaps, int* history, int* delay);
// Host only. taps[ntaps]: h[i] = rrc((i - (ntaps - 1) / 2) / sps - tau, rolloff) gain / (sum of the taps at tau = 0), designed in double,
// rounded once. tau in symbols, |tau| <= 0.5; rolloff in [0, 1]; gain finite and not zero. -1 on a bad argument
int pulse_taps(int sps, float rolloff, int rrc_delay, double tau, double gain, float* taps);
// Host only. The rule of scale_rrc_taps: every tap times sqrt(2) fullscale / max over p of sum over k of |h[p + k sps]|, in double,
// rounded once. -1 on a bad argument (no taps, sps < 1, a tap or fullscale that is not finite, taps that are all zero)
int pulse_scale_taps(float* taps, int ntaps, int sps, double fullscale);

class PulseShaperHip : public StreamStage {
public:
    PulseShaperHip(int sps, const float* taps, int ntaps, int max_streams, int max_symbols, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int sps, const float* taps, int ntaps, int max_streams, int max_symbols);
    int sps() const { return sps_; }
    int ntaps() const { return ntaps_; }
    int history() const { return history_; }
    int max_symbols() const { return max_samples(); } // the name the entry uses: a row of this stage is symbols
    int reset(); // synchronous: waits for the device, then clears every history
    // DEVICE pointers, 8-byte aligned, strides in complex elements; two launches, asynchronous on `stream`. The entry (c_api_pulse.hip)
    // checks the arguments. One call in flight per handle: the histories are read by a call and rewritten behind it, so a second call on
    // ANOTHER stream needs the first to have finished; calls on the same stream may follow each other.
    int shape_device(const float* d_in, int64_t in_stride, int n_syms, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream);

private:
    int sps_ = 0, ntaps_ = 0, history_ = 0;
    float* d_taps_ = nullptr;
    float2* d_hist_ = nullptr; // max_streams * history, the oldest symbol first
};

} // namespace dvbs2
