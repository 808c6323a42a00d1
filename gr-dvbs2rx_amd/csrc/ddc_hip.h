// ddc_hip.h -- digital down-conversion on the device: a frequency-translating decimating FIR (GNU Radio's freq_xlating_fir_filter_ccf, or
// a rotator followed by fir_filter_ccf with decimation; neither block is in the reference tree, so the stage is UNPINNED against it). One
// wideband capture, or a few, become C baseband streams: channel c reads input stream input[c], mixes it with its own phase increment,
// filters with the handle's real taps and keeps every D-th sample. What is pinned is the arithmetic, which tests/ddc_model.py restates
// and the device equals bit for bit.
//
// Mix: z[n] = x[n] e^{j phi_c(n)} with the rotator's arithmetic (rotator_math.hpp): the phase in turns as unsigned 64-bit fixed point,
// phi_c(n) = P_c + (n - n_call) I_c in wrapping integer arithmetic, I_c = rotator_inc_turns(inc[c]); no special case for inc == 0.
// Filter and decimate: output k (absolute, k >= 0) is y[k] = sum_{t = 0}^{ntaps - 1} h[t] z[k D - t], real and imaginary part apart, each
// term a float product and then a float addition (no contraction), t ascending, onto an accumulator that starts at +0.0f. z[n] for n < 0
// is zero after create / reset.
// Counts: all channels and inputs share one 64-bit sample counter n0. A call that consumes the absolute inputs [n0, n0 + n_in) writes the
// outputs k with n0 <= k D < n0 + n_in, n_out = ceil((n0 + n_in) / D) - ceil(n0 / D) for every channel, and leaves n0' = n0 + n_in and
// P_c' = P_c + n_in I_c for the channels of the call.
// State: per channel the last ntaps - 1 MIXED samples stay on the device, so the stage equals "rotator, then decimating FIR" bit for bit
// however the stream is cut into calls and whenever increments change between calls (set_channel; the phase stays continuous).
//
// Kernel: grid.x the channel (fastest, so that the channels of one input tile run close together and share its bytes in L2), grid.y
// tiles of ddc_tile(D, ntaps) consecutive OUTPUT samples. A block stages the tile's span of tile D + ntaps - 1 mixed samples in LDS --
// samples before the call come from the channel's history, already mixed; every other one is mixed once -- in POLYPHASE order: sample m of
// the span at row m mod D, column m div D. For a tap all lanes then read one row and consecutive lanes, which own consecutive outputs,
// consecutive columns: conflict-free 8-byte reads at any D. The taps are uniform and come through scalar loads; a lane owns up to four
// outputs, 256 apart, so that one tap serves them. A second, tiny launch behind the first writes each channel's new history and phase, so
// no block of the first can see them change.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kDdcMaxDecim = 256;
constexpr int kDdcMaxTaps = 4096;         // history <= 4095 samples: 16 per thread of the state launch
constexpr int kDdcMaxSamples = 1 << 24;   // inputs per stream and call
constexpr int kDdcSpan = 9216;            // mixed samples a block stages at most: 72 KiB, two workgroups per CU
constexpr int kDdcMaxTile = 1024;         // output samples per block at most: four per lane
constexpr int64_t kDdcMaxPosition = (int64_t)1 << 62; // the counter a call may start from at most: no sum of the count rule wraps

// Host only. Output samples per block: as many as keep tile D + ntaps - 1 within kDdcSpan, kDdcMaxTile at most (at least 20). No checks
inline int ddc_tile(int decim, int ntaps)
{
    const int fit = (kDdcSpan - (ntaps - 1)) / decim;
    return fit < kDdcMaxTile ? fit : kDdcMaxTile;
}
// Host only. history = ntaps - 1 mixed samples per channel; the signal is delayed by delay_num / 2 input samples, delay_num = ntaps - 1;
// each nullable. -1: decim outside 1..256 or ntaps outside 1..4096
int ddc_geometry(int decim, int ntaps, int* history, int* delay_num);
// Host only. What a call of n_in samples writes per channel when the counter stands at `position`:
// ceil((position + n_in) / decim) - ceil(position / decim). -1: position outside 0..kDdcMaxPosition, decim outside 1..256 or n_in outside
// 0..2^24
int64_t ddc_produce(int64_t position, int decim, int n_in);

// Host only: the counter and the phases as the device has them after every accepted call, in plain integer arithmetic
struct DdcMirror {
    int64_t counter = 0;
    std::vector<uint64_t> phase, inc; // per channel, 2^-64 turns
    void advance(int n_in, int n_channels)
    {
        for (int c = 0; c < n_channels; c++) phase[c] += (uint64_t)n_in * inc[c];
        counter += n_in;
    }
};

class DdcHip : public StreamStage {
public:
    DdcHip(int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples);
    int decim() const { return decim_; }
    int ntaps() const { return ntaps_; }
    int history() const { return ntaps_ - 1; }
    int tile() const { return tile_; }
    int max_channels() const { return max_streams(); } // the rows of this stage are its channels
    int max_inputs() const { return max_inputs_; }
    // host only: channel reads input stream `input` and advances by phase_inc radians per input sample from the next call on; the phase
    // is carried over. -1 (an argument error): channel or input out of range, phase_inc not finite
    int set_channel(int channel, int input, double phase_inc);
    int input_of(int channel) const { return table_[channel].input; }
    // host only, from the mirror: what the next call of n_in samples writes per channel
    int64_t produce(int n_in) const { return ddc_produce(mirror_.counter, decim_, n_in); }
    const DdcMirror& mirror() const { return mirror_; }
    int reset();                 // synchronous: waits for the device; counter 0, phases 0, histories zero, the channel table stays
    int state(uint64_t* phases); // synchronous: the device's phases, max_channels of them
    // DEVICE pointers, 8-byte aligned, strides in complex elements: channel c reads n_in samples at d_in + input[c] in_stride and writes
    // produce(n_in) samples at d_out + c out_stride. Two launches, asynchronous on `stream`; the first call behind a set_channel also
    // copies the channel table on `stream`. The entry (c_api_ddc.hip) checks the arguments, out_stride against produce() and every
    // channel's input against n_inputs among them. The mirror advances when both launches were accepted. One call in flight per handle:
    // histories and phases are read by a call and rewritten behind it.
    int process_device(const float* d_in, int64_t in_stride, int n_in, int n_channels, float* d_out, int64_t out_stride, hipStream_t stream);

    struct Chan { uint64_t inc; int32_t input, reserved; }; // a row of the channel table, on the device as on the host

private:
    int decim_ = 0, ntaps_ = 0, tile_ = 0, max_inputs_;
    DdcMirror mirror_;
    std::vector<Chan> table_;
    bool table_dirty_ = true;
    float* d_taps_ = nullptr;
    float2* d_hist_ = nullptr; // max_channels * history mixed samples, the oldest first
    unsigned long long* d_phase_ = nullptr;
    Chan* d_table_ = nullptr;
};

} // namespace dvbs2
