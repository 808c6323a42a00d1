// agc_hip.h -- automatic gain control on the device, the stage in front of the rotator (rotator_hip.h): in the reference's receive
// flowgraph (apps/dvbs2-rx:873-887) GNU Radio's analog.agc_cc(rate, reference, gain) with set_max_gain(65536) behind an optional
// blocks.swap_iq. GNU Radio is not in the reference tree, so the stage is UNPINNED against gr::analog::kernel::agc_cc::scale. What is
// pinned is the arithmetic, which tests/agc_model.py restates and the device equals bit for bit. Per stream, with float state g, for
// every sample x = (xr, xi) in order ((xi, xr) with swap_iq):
//   yr = xr * g ; yi = xi * g                   the output sample
//   m  = sqrt(yr * yr + yi * yi)                two products, one addition, a correctly rounded square root
//   g  = g + rate * (reference - m)             subtraction, product, addition
//   if (max_gain > 0 && g > max_gain) g = max_gain
// every operation one IEEE float32 operation in this order, nothing fused, denormals kept. No lower clamp and nothing special for
// values that are not finite: a NaN or an overflow propagates as IEEE arithmetic says (reset() is the way out). The square root is
// sqrtf, which hipcc expands to the correctly rounded sequence; __fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS the HIP
// headers map it to the native v_sqrt_f32, which is good to one ulp only (notes/agc.md).
//
// Kernel: the recurrence is serial in time, so the parallel axis is the batch of streams: ONE LANE PER STREAM. A workgroup is one
// wavefront that carries W streams (W = 8, 16 or 32 by the size of the batch: as few per wavefront as still leaves every SIMD of the
// device a wavefront or two, see agc_lanes) and walks them in tiles of kAgcTile samples. A tile of W rows is staged in LDS: all 64
// lanes load it along the rows, 16 bytes per lane (8 where a row does not start 16-byte aligned -- the same bits), every lane below W
// then walks its own row, 4 samples per trip through 16-byte LDS reads and writes, results go back into the tile and leave as they
// came. The row pitch is kAgcTile complex + 2: 4 dwords more than a multiple of 64, so the 16 lanes of one ds_read_b128 / the 8 of
// one ds_write_b128 hit different banks; the gains (asked for or not) have a tile of their own with pitch kAgcTile + 4 floats. The
// global loads of the NEXT tile are issued into registers before the current one is walked.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kAgcTile = 64; // samples per stream and tile

// Host only. Empty when the parameters are acceptable, else what is wrong with them: the text names the argument. max_gain == 0: no cap
std::string agc_check(float rate, float reference, float gain, float max_gain);
// Host only. Streams per wavefront for a batch of n_streams: the smallest of 8, 16, 32 that needs at most 2048 wavefronts
int agc_lanes(int n_streams);

class AgcHip : public StreamStage {
public:
    AgcHip(float rate, float reference, float gain, float max_gain, int max_streams, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(float rate, float reference, float gain, float max_gain, int max_streams, int max_samples);
    float rate() const { return rate_; }
    float reference() const { return reference_; }
    float max_gain() const { return max_gain_; }
    bool swap_iq() const { return swap_iq_; }
    int set_params(float rate, float reference, float max_gain); // host side: calls made after it
    void set_swap_iq(bool enable) { swap_iq_ = enable; }
    int reset();                             // synchronous: waits for the device, then every stream's gain is the constructor's
    int set_gain(int stream_index, float g); // synchronous; -1: every stream
    int state(float* gains, int n_streams);  // waits for the device
    // DEVICE pointers, samples 8-byte and gains 4-byte aligned, strides in elements; d_gain nullable; d_out == d_in with equal strides
    // is allowed. One launch, asynchronous on `stream`. The entry (c_api_agc.hip) checks the arguments. One call in flight per
    // handle: a call reads the gains and writes them back.
    int work_device(const float* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out, int64_t out_stride, float* d_gain,
                    int64_t gain_stride, hipStream_t stream);

private:
    int fill(int first, int count, float g);
    float rate_ = 0, reference_ = 0, gain0_ = 0, max_gain_ = 0;
    bool swap_iq_ = false;
    float* d_state_ = nullptr; // max_streams gains
};

} // namespace dvbs2
