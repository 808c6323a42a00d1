// pfbsyn_hip.h -- a polyphase SYNTHESIS filter bank on the device (GNU Radio's pfb_synthesizer_ccf; the block is not in the reference
// tree, so the stage is UNPINNED against it): the transpose of pfbch_hip.h. The rows of M equally spaced channels become one wideband
// stream at L times their rate, each row shaped by the handle's real taps as an interpolating FIR by L and moved to +c / M of the
// output rate, with ONE M-point inverse transform per input instant in place of M mixers and ONE FIR pass for all channels. What is
// pinned is the arithmetic, which tests/pfbsyn_model.py restates and the device equals bit for bit.
//
// Counts: one 64-bit counter k0 of input INSTANTS for all streams. A call of n_in instants reads n_in samples of each of the n_sel rows
// of a stream and writes the n_in L absolute outputs [k0 L, (k0 + n_in) L) of that stream; then k0' = k0 + n_in, at most 2^54.
// Transform: v[k][r] = sum_c a[c] e^{+2 pi j c r / M}, unnormalised, on the forward graph of spectrum_hip.h / pfbch_hip.h over the table
// of fft_twiddles.h with real and imaginary part exchanged on the way in and on the way out: the graph's input is (a.im, a.re) at the
// bit-reversed place of c, stage 1 without a product, every later stage Tr = Wr br - Wi bi, Ti = Wr bi + Wi br for every index, and
// (v.im, v.re) is what the graph returns. A channel without a row is +0.0f in both parts.
// FIR: for the absolute output n with r = n mod M, p = n mod L, k1 = n div L: acc = acc + h[p + j L] * v[k1 - j][r] over the j with
// p + j L <= ntaps - 1 and k1 - j >= 0, j DESCENDING (the oldest instant first), from +0.0f, the parts apart, a float product and then a
// float addition. An instant that does not exist is skipped.
// State: per stream the tail, max(ntaps - L, 0) partial sums: tail[i] is the acc of output k0 L + i over the instants below k0. The next
// call starts those outputs from it, so any cutting gives the bits of one call.
//
// Kernel: grid.x tiles of pfbsyn_tile(M, L, ntaps) consecutive instants, grid.y the stream; the instants run to n_in + q - 1,
// q = ceil(ntaps / L): the outputs of the q - 1 instants behind the call are the new tail (the instants themselves do not exist and are
// not transformed). A block transforms its tile's instants and the q - 1 before them (those of them inside the call) into an LDS store
// [instant][seg_len(M)], one pad element per 16 and an odd length as in pfbch_hip.hip; the taps sit behind the store.
// M <= 16: a lane owns an instant and transforms it in registers. M >= 32: the rows go to the bit-reversed places of the store, and the
// stages run in place in two register-blocked passes with a barrier between them (this file's own copy of the stage code, see
// notes/shared_stream_device.md). Then a lane owns an output sample: consecutive lanes read consecutive r of one instant, the instant
// stepping every L lanes, and consecutive taps p + j L, and store consecutive samples. An output below the tail's length starts from the
// old tail; an output at or past n_in L goes to the NEXT tail, a buffer of its own, and a second, tiny launch behind the first copies
// that buffer over the tails of the call's streams: no block can read a tail that another block of the same call has rewritten, and
// the tail of a stream that a call leaves out stays.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kPfbsynMinLog2 = 1, kPfbsynMaxLog2 = 8; // M = 2..256
constexpr int kPfbsynMaxChan = 1 << kPfbsynMaxLog2;
constexpr int kPfbsynMaxTaps = 4096;
constexpr int kPfbsynMaxSamples = 1 << 24;      // input instants per row and call
constexpr int kPfbsynMaxOut = 1 << 28;          // max_samples * interp at most
constexpr int kPfbsynMaxProduct = 8192;         // n_chan * ceil(ntaps / interp) at most: the transformed instants before a tile stay on chip
constexpr int kPfbsynSpan = 6144;               // complex elements of the LDS store a block takes when its tile then is at least q: 48 KiB
constexpr int kPfbsynSpanLong = 13312;          // ... and otherwise (long filters on few phases): 104 KiB, one workgroup per CU
constexpr int kPfbsynMaxTile = 512;             // instants per block at most
constexpr int kPfbsynRegisterLog2 = 4;          // M <= 16: the transform in a lane's registers
constexpr int64_t kPfbsynMaxPosition = (int64_t)1 << 54;

// Host only. log2 of n_chan, or -1 when it is no power of two in 2..256
int pfbsyn_log2(int n_chan);
// Host only. Elements of one instant in the LDS store: M and one pad element per 16, made odd
constexpr int pfbsyn_seg_len(int n_chan) { return (n_chan + (n_chan >> 4)) | 1; }
// Host only. Input instants per block: the store holds tile + q - 1 instants, q = ceil(ntaps / interp), within kPfbsynSpan elements where
// that leaves a tile of at least q, within kPfbsynSpanLong otherwise; kPfbsynMaxTile at most. At least 12 (M 256, q 11) for every shape that
// creation accepts. No checks
inline int pfbsyn_tile(int n_chan, int interp, int ntaps)
{
    const int q = (ntaps + interp - 1) / interp, seg = pfbsyn_seg_len(n_chan);
    int fit = kPfbsynSpan / seg - (q - 1);
    if (fit < q) fit = kPfbsynSpanLong / seg - (q - 1);
    return fit < kPfbsynMaxTile ? fit : kPfbsynMaxTile;
}
// Host only. tail = max(ntaps - interp, 0) partial sums per stream; the signal is delayed by delay_num / 2 OUTPUT samples, delay_num =
// ntaps - 1; taps_per_phase = ceil(ntaps / interp); each nullable. -1: n_chan no power of two in 2..256, interp outside 1..n_chan or
// ntaps outside 1..4096
int pfbsyn_geometry(int n_chan, int interp, int ntaps, int* tail, int* delay_num, int* taps_per_phase);
// Host only. The counter behind a call of n_in instants that starts at `position`, or -1: position outside 0..2^54, n_in outside
// 0..2^24, or the sum above 2^54
int64_t pfbsyn_advance(int64_t position, int n_in);

class PfbsynHip : public StreamStage {
public:
    PfbsynHip(int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples);
    // empty when list[0 .. n_sel) is acceptable for n_chan channels: 1..n_chan distinct indices below n_chan
    static std::string check_channels(int n_chan, const int* list, int n_sel);
    int n_chan() const { return n_chan_; }
    int interp() const { return interp_; }
    int ntaps() const { return ntaps_; }
    int tail() const { return tail_; }
    int tile() const { return tile_; }
    int64_t position() const { return counter_; }
    const std::vector<int32_t>& channels() const { return list_; }
    // host only: from the next call on row i feeds channel list[i]. -1 (an argument error): see check_channels
    int set_channels(const int* list, int n_sel);
    // host only, from the mirror: what the next call of n_in instants writes per stream, or -1 when the counter would pass 2^54
    int64_t produce(int n_in) const { return pfbsyn_advance(counter_, n_in) < 0 ? -1 : (int64_t)n_in * interp_; }
    int reset(); // synchronous: waits for the device; counter 0, tails zero, the selection stays
    // DEVICE pointers, 8-byte aligned, strides in complex elements: row i of stream s is n_in samples at d_in + (s n_sel + i) in_stride,
    // stream s writes n_in interp samples at d_out + s out_stride. Two launches at most, asynchronous on `stream`; the first call behind
    // a set_channels also copies the selection on `stream`. The entry (c_api_pfbsyn.hip) checks the arguments and out_stride. The
    // mirror advances when both launches were accepted. One call in flight per handle. "A refused call changes nothing" holds for
    // every refusal of the checks; it does NOT cover a device error between the two launches: the call then returns -1 (kDevice) with
    // the outputs written, the tails as they were and the counter not advanced, and the handle is to be reset.
    int process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream);

private:
    int n_chan_ = 0, log2_ = 0, interp_ = 0, ntaps_ = 0, tail_ = 0, q_ = 0, tile_ = 0;
    int64_t counter_ = 0;
    std::vector<int32_t> list_;  // the selection
    std::vector<int32_t> table_; // what the device reads: the row of every channel or -1
    bool table_dirty_ = true;
    float* d_taps_ = nullptr;
    float2* d_twiddles_ = nullptr; // the table's entries in stage order, n_chan - 1 of them
    float2* d_tail_ = nullptr;     // max_streams * tail partial sums, then as many for the tails a call leaves
    int32_t* d_table_ = nullptr;
};

} // namespace dvbs2
