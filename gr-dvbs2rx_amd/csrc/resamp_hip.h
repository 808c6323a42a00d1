// resamp_hip.h -- arbitrary-rate resampling on the device: a polyphase filter bank of `nfilts` branches with linear interpolation between
// neighbouring branches through a bank of derivative taps, real taps over complex samples, on a batch of independent streams whose
// histories and positions stay on the device between calls. In the reference's transmit flowgraph (apps/dvbs2-tx:641-686) it is the
// fractional-sps branch, GNU Radio's pfb_arb_resampler_ccf(sps, rrc_taps) with 32 branches; the block is not in the reference tree, so the
// stage is UNPINNED against it. What is pinned is the arithmetic, which tests/resamp_model.py restates and the device equals bit for bit.
//
// Position: `step` counts input samples per output sample with 32 fractional bits; the rate is exactly 2^32 / step. Each stream has a
// 64-bit `acc`. Output m of a call that takes n_in samples sits at T = acc + m step; the call produces every m with T < N = n_in << 32,
// that is n_out = 0 if acc >= N, else ceil((N - acc) / step), and leaves acc' = acc + n_out step - N. From T: i = T >> 32 is the newest
// input sample used (0-based in this call's input), f = T & 0xffffffff the fraction, j = f >> (32 - log2 nfilts) the branch and
// a = float((f << log2 nfilts) >> 8) * 2^-24 the weight of the derivative bank (32-bit words; the conversion is exact).
// Arithmetic: d[n] = h[n + 1] - h[n], d[ntaps - 1] = 0, made once in float32. For an output at (i, j, a), real and imaginary part apart:
//   o0 = sum_k h[j + k nfilts] x[i - k],  o1 = sum_k d[j + k nfilts] x[i - k],  k ascending from 0 while j + k nfilts < ntaps,
//   each term a float product and then a float addition (no contraction) onto an accumulator that starts at +0.0f; y = o0 + a * o1.
// x before the call is the stream's history: L - 1 samples, L = ceil(ntaps / nfilts), zeros after create / reset.
//
// Kernel: grid.y the stream, grid.x tiles of kResampTile consecutive OUTPUT samples. A block derives the input span of its tile from the
// stream's acc, step and the tile index in 64-bit scalar arithmetic, stages that span and the L - 1 samples before it in LDS (samples
// before the call come from the history buffer) and the bank of {h, d} pairs behind it. Consecutive lanes own consecutive outputs. A
// second, tiny launch behind the first writes each stream's new history and position, so no block of the first can see them change.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kResampTile = 1024;    // output samples per block
constexpr int kResampMaxTerms = 128; // L at most: history <= 127 samples, one block of the state launch
constexpr int kResampMaxTaps = 8192;
constexpr int kResampMaxSamples = 1 << 24; // inputs per stream and call: N = n_in << 32 and everything added to it stay below 2^58
constexpr uint64_t kResampMinStep = 1ull << 26, kResampMaxStep = 1ull << 33; // rates 64 and 0.5

// Host only. step = nearbyint(2^32 / rate) in double for rate in [0.5, 64]. -1: any other rate (NaN included) or a null step
int resamp_step(double rate, uint64_t* step);
// Host only. L = ceil(ntaps / nfilts) terms, history = L - 1 samples, delay_num = (ntaps - 1) / 2: the signal is delayed by
// delay_num / nfilts input samples; each nullable. -1: nfilts is not a power of two in 2..256, ntaps not in 1..8192, or L > 128
int resamp_geometry(int nfilts, int ntaps, int* L, int* history, int* delay_num);
// Host only. What one stream at `acc` writes for n_in samples in, and where it stands afterwards (nullable). No checks: acc < 2^34,
// step in [2^26, 2^33], 0 <= n_in <= 2^24 is the caller's to see to
inline int64_t resamp_advance(uint64_t acc, uint64_t step, int n_in, uint64_t* acc_after)
{
    const uint64_t N = (uint64_t)n_in << 32;
    const uint64_t n = acc >= N ? 0 : (N - acc + step - 1) / step;
    if (acc_after) *acc_after = acc + n * step - N;
    return (int64_t)n;
}
// Host only. The largest n_out of a call of n_in samples for any acc: ceil((n_in << 32) / step). -1: step outside [2^26, 2^33] or n_in
// outside 0..2^24
int64_t resamp_max_out(uint64_t step, int n_in);

class ResamplerHip : public StreamStage {
public:
    ResamplerHip(int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples);
    int nfilts() const { return nfilts_; }
    int ntaps() const { return ntaps_; }
    int terms() const { return L_; }
    int history() const { return L_ - 1; }
    uint64_t step() const { return step_; }
    // host only: the next call uses it, acc is carried over. -1 (an argument error): step outside [2^26, 2^33]
    int set_step(uint64_t step);
    // host only, from the mirror: what the next call of n_in samples writes for streams 0 .. n_streams; returns the largest
    int64_t produce(int n_in, int n_streams, int64_t* n_out) const;
    int reset();                           // synchronous: waits for the device, then clears every history and position
    int reset_phase(const uint32_t* frac); // synchronous: acc[s] = frac[s] for every stream of the handle (null: zeros); histories stay
    int state(uint64_t* acc);              // synchronous: the device's positions, max_streams of them
    const std::vector<uint64_t>& mirror() const { return acc_; }
    // DEVICE pointers, 8-byte aligned, strides in complex elements; two launches, asynchronous on `stream`. The entry (c_api_resamp.hip)
    // checks the arguments, out_stride against produce() among them. The mirror advances when both launches were accepted. One call in
    // flight per handle: histories and positions are read by a call and rewritten behind it.
    int process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream);

private:
    int nfilts_ = 0, lg_ = 0, ntaps_ = 0, L_ = 0, row_ = 0, bank_elems_ = 0;
    uint64_t step_ = 0;
    std::vector<uint64_t> acc_; // the host's mirror of d_acc_: plain integer arithmetic, advanced at every accepted call
    float2* d_bank_ = nullptr;  // {h, d} per [branch][term], rows of row_ = L | 1 pairs, zeros where a branch has no tap
    float2* d_hist_ = nullptr;  // max_streams * history, the oldest sample first
    unsigned long long* d_acc_ = nullptr;
};

} // namespace dvbs2
