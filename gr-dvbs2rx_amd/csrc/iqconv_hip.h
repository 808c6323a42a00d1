// iqconv_hip.h -- the IQ sample converter on the device, the stage at the very ends of both flowgraphs: in the reference's receive
// flowgraph (apps/dvbs2-rx:685-707) blocks.deinterleave / uchar_to_float / add_const(-127.5) / multiply_const(1/128) / float_to_complex
// in front of the AGC, in its transmit flowgraph (apps/dvbs2-tx:533-549, apps/dvbs2-rec:439-446) complex_to_float / multiply_const(128) /
// add_const(127.5) / float_to_uchar / interleave behind the last filter, and the level reading blocks.rms_cf gives the GUI
// (apps/dvbs2-rx:952) in its block-mean form. GNU Radio is not in the reference tree, so the stage is UNPINNED against those blocks. What
// is pinned is the arithmetic (iqconv_math.hpp), which tests/iqconv_model.py restates and the device and the host restatement equal
// bit for bit. Formats: u8 (RTL-SDR, the reference's recorder), s8 (HackRF), s16 in host byte order (USRP, bladeRF, Pluto).
//
// NO DEVICE STATE. The handle holds the format, the gain and the checked limits; the statistics live in the caller's buffer and are
// added to with atomics. ANY NUMBER OF CALLS MAY BE IN FLIGHT PER HANDLE.
//
// Kernels: one launch per direction, templated on the format, on the aligned / edge path and on whether statistics are wanted. The work
// is cut into PIECES of four components (two complex samples): 16 bytes on the float side, a dword (u8, s8) or 8 bytes (s16) on the
// code side. Neighbouring lanes take neighbouring pieces; a lane takes kIqPieces of them, in batches (8 in unpack, 4 in pack) with the loads of a
// batch in front of its stores. A piece is always STORED whole and aligned:
//   unpack  pieces are aligned on the float side (a 16-byte store). Wide path: the codes are one aligned load. Edge path: the aligned
//           dwords that hold the piece's codes are loaded and shifted together by the row's byte phase.
//   pack    wide path: a 16-byte load, an aligned code store. Edge path: pieces are aligned on the code side (an aligned dword or 8-byte
//           store); the four floats come as two 8-byte or, at an odd component, four 4-byte loads.
// A piece that is cut by the row's ends, or whose aligned code dwords would reach outside the row, goes component by component with
// byte or short accesses on the code side: nothing outside [0, n) of a row is read or written. Statistics: per lane in registers, per
// wave by shuffles, per workgroup through LDS, then one atomicAdd per counter and workgroup (none for a zero; the row's samples by its
// first workgroup).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kIqLanes = 256, kIqPieces = 16;
constexpr int kIqconvTile = kIqLanes * kIqPieces * 2; // samples of a row one workgroup covers

// Host only. Bytes per complex sample, -1 for an unknown format.
int iqconv_bytes(int format);
// Host only. Empty when acceptable, else what is wrong: the text names the argument.
std::string iqconv_check(int format, float gain, int max_streams, int max_samples);
// Host only: the host compilation of iqconv_math.hpp over n samples at any address; stats nullable, {samples, clipped, energy} ADDED.
void iqconv_unpack_host(int format, float gain, const void* in, int64_t n, float* out, uint64_t* stats);
void iqconv_pack_host(int format, float gain, const float* in, int64_t n, void* out, uint64_t* stats);

class IqconvHip : public StreamStage {
public:
    IqconvHip(int format, float gain, int max_streams, int max_samples, int device);
    int format() const { return format_; }
    float gain() const { return gain_; }
    int set_gain(float gain); // host side: calls made after it
    // DEVICE pointers, strides in complex samples; codes at any byte address (s16: any even one), floats 8-byte aligned, d_stats
    // nullable (n_streams x 3 uint64, added to). One launch, asynchronous on `stream`, no allocation and no synchronisation. The
    // entries (c_api_iqconv.hip) check the arguments.
    int unpack_device(const void* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out, int64_t out_stride, uint64_t* d_stats,
                      hipStream_t stream);
    int pack_device(const float* d_in, int64_t in_stride, int n_samples, int n_streams, void* d_out, int64_t out_stride, uint64_t* d_stats,
                    hipStream_t stream);

private:
    int format_ = 0;
    float gain_ = 1.0f;
};

} // namespace dvbs2
