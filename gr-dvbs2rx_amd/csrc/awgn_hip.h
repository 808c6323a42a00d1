// awgn_hip.h -- the additive white Gaussian noise channel on the device, the stage behind the pulse shaper (pulse_hip.h) and in front of
// the rotator: in the reference's transmit flowgraph (apps/dvbs2-tx:572-584) GNU Radio's analog.noise_source_c(GR_GAUSSIAN,
// sqrt(N0 * sps)) into blocks.add_vcc. GNU Radio is not in the reference tree, so the stage is UNPINNED against
// gr::analog::noise_source_c, whose generator is another one. What is pinned is the arithmetic (awgn_math.hpp), which
// tests/awgn_model.py restates and the device and the host restatement equal bit for bit: the noise of a sample is a pure function of
// (seed, stream id, absolute sample index), Philox4x32-10 words through a float32 Box-Muller, and y = x + sigma * noise per component.
//
// NO DEVICE STATE. The handle holds the seed, the scalar sigma and the checked limits, nothing lives on the device between calls and a
// call reads nothing but its arguments. So, unlike the AGC and the pulse shaper (one call in flight per handle), ANY NUMBER OF CALLS
// MAY BE IN FLIGHT PER HANDLE, on any streams, and however a stream is cut into calls the bits are those of one call: the caller says
// where a call stands (first_stream, first_index).
//
// Kernel: one launch, no LDS. A lane owns one generator block: absolute samples 2 b and 2 b + 1 of its row, one Philox call, two
// Box-Muller pairs, one 16-byte load and one 16-byte store where the block's address is 16-byte aligned in every row (kWide), else two
// 8-byte accesses with the same bits. A call that starts or ends on an odd absolute index has a half block at that edge. Grid:
// (generator blocks of a row / 256, rows); sigma is a kernel argument or, with d_sigma, one load per row.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kAwgnTile = 512; // samples of a row one workgroup covers: 256 lanes, one generator block each

// Host only. Empty when acceptable, else what is wrong: the text names the argument.
std::string awgn_check(float sigma, int max_streams, int max_samples);
// Host only. Per-component standard deviation for Es/N0 in dB, symbol energy es and sps samples per symbol: N0 = es / 10^(esn0_db/10),
// sigma = sqrt(N0 sps / 2), in double, rounded once (apps/dvbs2-tx:574-580). Empty, or what is wrong.
std::string awgn_sigma(double esn0_db, double es, int sps, float* sigma);
// Host only: the host compilation of awgn_math.hpp. (wa, wb) and the unit-variance noise (re, im) of one sample.
void awgn_words(uint64_t seed, uint64_t stream_id, int64_t index, uint32_t* wa_wb);
void awgn_sample(uint64_t seed, uint64_t stream_id, int64_t index, float* re_im);

class AwgnHip : public StreamStage {
public:
    AwgnHip(uint64_t seed, float sigma, int max_streams, int max_samples, int device);
    uint64_t seed() const { return seed_; }
    float sigma() const { return sigma_; }
    int set_sigma(float sigma); // host side: calls made after it
    void set_seed(uint64_t seed) { seed_ = seed; }
    // DEVICE pointers, samples 8-byte aligned, strides in complex elements; d_in nullable (noise only), d_sigma nullable (n_streams
    // floats, replaces the handle's sigma, not checked); d_out == d_in with equal strides is allowed. One launch, asynchronous on
    // `stream`, no allocation and no synchronisation. The entry (c_api_channel.hip) checks the arguments.
    int add_device(const float* d_in, int64_t in_stride, int n_samples, int n_streams, uint64_t first_stream, int64_t first_index,
                   const float* d_sigma, float* d_out, int64_t out_stride, hipStream_t stream);

private:
    uint64_t seed_;
    float sigma_ = 0;
};

} // namespace dvbs2
