// pfbch_hip.h -- a polyphase filter bank channelizer on the device (GNU Radio's pfb_channelizer_ccf; the block is not in the reference
// tree, so the stage is UNPINNED against it): one wideband capture becomes M equally spaced channels, each filtered by the handle's real
// taps and decimated by D, with the FIR work done ONCE for all channels and one M-point transform in place of M mixers. What is pinned
// is the arithmetic, which tests/pfbch_model.py restates and the device equals bit for bit.
//
// Counts: the down-converter's (ddc_hip.h). One 64-bit sample counter n0 for all streams; a call over the absolute inputs
// [n0, n0 + n_in) writes the outputs k with n0 <= k D < n0 + n_in, n_out = ceil((n0 + n_in) / D) - ceil(n0 / D), and leaves n0 + n_in.
// Branch sums: for output k and residue r in 0..M-1, w[k][r] = sum over the taps t with (k D - t) mod M == r of h[t] x[k D - t], t
// ascending, real and imaginary part apart, each term a float product and then a float addition onto +0.0f, nothing contracted; a
// residue without a tap is +0.0f. The residue is that of the ABSOLUTE sample index, so D need not divide M and cuts do not matter.
// x[n] for n < 0 is zero after create / reset.
// Transform: Y[k][c] = sum_r w[k][r] e^{-2 pi j c r / M} by the radix-2 graph of spectrum_hip.h over the table of fft_twiddles.h:
// input to bit-reversed places, stage 1 without a product, every later stage Tr = Wr br - Wi bi, Ti = Wr bi + Wi br for every index.
// Channel c is the band centred at +c / M of the input rate: in exact arithmetic dvbs2_ddc_* with phase_inc = -2 pi c / M.
// Output: row i of stream s is n_out complex samples at d_out + (s n_sel + i) out_stride and holds channel list[i] of the selection
// (set_channels; all M ascending until set). Channels that are not selected are not written.
// State: per stream the last ntaps - 1 RAW samples. No phases.
//
// Kernel: grid.x tiles of pfbch_tile(M, D, ntaps) consecutive OUTPUT instants, grid.y the stream. A block stages the tile's span of raw
// samples in LDS in polyphase order BY M -- the sample of absolute index n at row n mod M, column n div M (from a multiple of M at or
// below the oldest sample the tile needs) -- and the taps behind them. The taps of a branch sum then meet one row at descending columns.
// M <= 16: a lane owns an output instant, forms its M branch sums over ascending q (tap p + q M, p = (k D - r) mod M its own: the taps
// come from LDS, not through scalar loads) and runs the transform in registers; consecutive lanes read one row at equal or consecutive
// columns (D <= M) and store consecutive samples of a channel's row.
// M >= 32: batches of 2048 / M instants. A lane forms the branch sums of (instant, residue) pairs, consecutive lanes consecutive
// residues -- consecutive rows of one column, an odd column count apart -- and puts them at their bit-reversed places of a scratch
// segment in LDS; the stages run in two register-blocked passes (8 or 16 points per lane, 4 at M = 32 in the second) with an LDS
// exchange, as in spectrum_hip.hip; the result goes back to the segment and is stored row by row, consecutive lanes consecutive instants.
// A second, tiny launch behind the first writes each stream's new history, so no block of the first can see it change.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kPfbchMinLog2 = 1, kPfbchMaxLog2 = 8; // M = 2..256
constexpr int kPfbchMaxChan = 1 << kPfbchMaxLog2;
constexpr int kPfbchMaxTaps = 4096;        // history <= 4095 samples: 16 per thread of the state launch
constexpr int kPfbchMaxSamples = 1 << 24;  // inputs per stream and call
constexpr int kPfbchSpan = 5376;           // raw samples a block stages at most, the alignment to M included: with the taps (16 KiB at
                                           // most) and the scratch segments (17.5 KiB) below 80 KiB, two workgroups per CU
constexpr int kPfbchMaxTile = 1024;        // output instants per block at most
constexpr int kPfbchBatchPoints = 2048;    // M >= 32: points of the instants that are transformed side by side
constexpr int kPfbchRegisterLog2 = 4;      // M <= 16: branch sums and transform in a lane's registers
constexpr int64_t kPfbchMaxPosition = (int64_t)1 << 62;

// Host only. log2 of n_chan, or -1 when it is no power of two in 2..256
int pfbch_log2(int n_chan);
// Host only. Output instants per block: as many as keep (tile - 1) D + ntaps - 1 + M within kPfbchSpan, kPfbchMaxTile at most (at least
// 4). No checks
inline int pfbch_tile(int n_chan, int decim, int ntaps)
{
    const int fit = (kPfbchSpan - (ntaps - 1) - n_chan) / decim;
    return fit < kPfbchMaxTile ? fit : kPfbchMaxTile;
}
// Host only. history = ntaps - 1 raw samples per stream; the signal is delayed by delay_num / 2 input samples, delay_num = ntaps - 1;
// taps_per_branch = ceil(ntaps / n_chan); each nullable. -1: n_chan no power of two in 2..256, decim outside 1..n_chan or ntaps
// outside 1..4096
int pfbch_geometry(int n_chan, int decim, int ntaps, int* history, int* delay_num, int* taps_per_branch);
// Host only. The count rule: ceil((position + n_in) / decim) - ceil(position / decim). -1: position outside 0..2^62, decim outside
// 1..256 or n_in outside 0..2^24
int64_t pfbch_produce(int64_t position, int decim, int n_in);
// Host only. The n_chan / 2 table entries as (re, im) pairs: spectrum_twiddles for 2..256. -1: n_chan out of range or out null
int pfbch_twiddles(int n_chan, float* out);

class PfbchHip : public StreamStage {
public:
    PfbchHip(int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples);
    // empty when list[0 .. n_sel) is acceptable for n_chan channels: 1..n_chan distinct indices below n_chan
    static std::string check_channels(int n_chan, const int* list, int n_sel);
    int n_chan() const { return n_chan_; }
    int decim() const { return decim_; }
    int ntaps() const { return ntaps_; }
    int history() const { return ntaps_ - 1; }
    int tile() const { return tile_; }
    int64_t position() const { return counter_; }
    const std::vector<int32_t>& channels() const { return list_; }
    // host only: from the next call on row i holds channel list[i]. -1 (an argument error): see check_channels
    int set_channels(const int* list, int n_sel);
    // host only, from the mirror: what the next call of n_in samples writes per channel
    int64_t produce(int n_in) const { return pfbch_produce(counter_, decim_, n_in); }
    int reset(); // synchronous: waits for the device; counter 0, histories zero, the selection stays
    // DEVICE pointers, 8-byte aligned, strides in complex elements: stream s reads n_in samples at d_in + s in_stride and writes
    // produce(n_in) samples per selected channel at d_out + (s n_sel + i) out_stride. Two launches, asynchronous on `stream`; the first
    // call behind a set_channels also copies the selection on `stream`. The entry (c_api_pfbch.hip) checks the arguments and out_stride
    // against produce(). The mirror advances when both launches were accepted. One call in flight per handle: the histories are read by a
    // call and rewritten behind it. "A refused call changes nothing" holds for every refusal of the checks. It does NOT cover a device
    // error between the two launches: if the runtime accepts the main launch and refuses the state launch, the call returns -1 (kDevice)
    // with the outputs written, the histories as they were and the counter not advanced; the handle is then to be reset.
    int process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream);

private:
    int n_chan_ = 0, log2_ = 0, decim_ = 0, ntaps_ = 0, tile_ = 0;
    int64_t counter_ = 0;
    std::vector<int32_t> list_;  // the selection
    std::vector<int32_t> table_; // what the device reads: list_ padded to kPfbchMaxChan, then the row of every channel or -1
    bool table_dirty_ = true;
    float* d_taps_ = nullptr;
    float2* d_twiddles_ = nullptr; // the table's entries in stage order, n_chan - 1 of them
    float2* d_hist_ = nullptr;     // max_streams * history raw samples, the oldest first
    int32_t* d_table_ = nullptr;
};

} // namespace dvbs2
