// spectrum_hip.h -- power spectra of sample streams on the device (Welch's averaged periodogram: what GNU Radio's freq_sink_c and
// waterfall_sink_c show; neither is in the reference tree, so the stage is UNPINNED against it) and, on the host, a carrier finder over
// one row of such a spectrum. What is pinned is the arithmetic, which tests/spectrum_model.py restates and the device equals bit for bit.
//
// Segments: segment s of a stream is the call's samples [s hop, s hop + nfft); n_seg = (n_in - nfft) / hop + 1 for n_in >= nfft, else 0.
// With avg > 0 a row is avg consecutive segments (n_rows = n_seg / avg, what is left over is not used); with avg == 0 the call's segments
// form one row. The handle holds no signal state: a call is a pure function of its input.
// Window: xw = (re w[n], im w[n]), one float product each.
// Transform: X[k] = sum_n xw[n] e^{-2 pi j k n / nfft} as the radix-2 decimation-in-time graph over the input in bit-reversed order:
// stage s = 1..t pairs the indices i and i + 2^(s-1) (bit s-1 of i clear), (a, b) -> (a + T, a - T), T = W b, W entry
// (i mod 2^(s-1)) nfft / 2^s of ONE table of nfft / 2 entries (float(cos(2 pi i / nfft)), float(-sin(2 pi i / nfft))), evaluated in
// double on the host. Stage 1 has no product (T = b); every later stage does Tr = Wr br - Wi bi, Ti = Wr bi + Wi br for every index,
// two float products and one float addition each, nothing contracted.
// Power: p = Xr Xr + Xi Xi. Averaging: the segments of a row in chunks of kSpectrumChunk consecutive segments (the last may be shorter);
// a chunk's sum per bin is float additions in ascending segment order onto +0.0f, the row is the chunk sums added in ascending order onto
// +0.0f, then one float product with scale = float(1 / (n sum_n w[n]^2)), n the row's segment count, the sum of squares in double in
// ascending n.
// Output: row r of stream i is nfft floats at d_out + i out_stride + r nfft; bins 0..nfft-1 (DC first), or with `shifted`
// nfft/2..nfft-1, 0..nfft/2-1 (DC at index nfft/2).
//
// Kernel: one workgroup of 256 threads per (stream, row, chunk). It walks the chunk's segments with the segment in LDS (nfft complex
// floats, one pad element per 16: 68 KiB at 8192, two workgroups per CU): the windowed samples go to their bit-reversed positions, then
// the stages run in register-blocked passes of 3 or 4 stages (8 or 16 points per lane) with an LDS exchange between passes; the last
// pass leaves the power in the lane's registers, which carry the chunk's sums and are stored once. At nfft <= 1024 a segment has fewer
// groups than the workgroup has lanes: 16 (nfft <= 256), 4 (512) or 2 (1024) segments of the chunk run side by side, their powers meet
// in LDS and are added in segment order. Where a row is one chunk the kernel writes the scaled row itself; else the chunk sums go to the
// handle's scratch buffer and a second, tiny launch behind the first adds them in order, scales and writes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "stream_stage.h"

namespace dvbs2 {

constexpr int kSpectrumChunk = 16;            // segments whose powers one workgroup adds in order
constexpr int kSpectrumMinLog2 = 6, kSpectrumMaxLog2 = 13;
constexpr int kSpectrumMaxHop = 1 << 24;
constexpr int kSpectrumMaxSamples = 1 << 24;  // per stream and call
enum SpectrumWindow { kSpectrumRect = 0, kSpectrumHann = 1, kSpectrumHamming = 2, kSpectrumBlackmanHarris = 3 };

// Host only. The counts of a call of n_in samples per stream, each nullable; used_samples: one past the last sample a row reads.
// -1: nfft no power of two in 64..8192, hop outside 1..2^24, avg negative or n_in outside 0..2^24
int spectrum_geometry(int nfft, int hop, int avg, int n_in, int* n_seg, int* n_rows, int* used_samples);
// Host only. The periodic window of `kind` (a SpectrumWindow), evaluated in double and rounded once. -1: kind or nfft out of range
int spectrum_window(int kind, int nfft, float* out);
// Host only. The nfft / 2 table entries as (re, im) pairs. -1: nfft out of range
int spectrum_twiddles(int nfft, float* out);
// Host only. sum_n w[n]^2 in double, ascending n
double spectrum_window_power(const float* window, int nfft);

// Host only: the carrier finder over one row (spectrum_carriers.cpp)
struct SpectrumCarrierParams { double floor_quantile, threshold_db; int32_t smooth, min_gap, min_width, reserved; };
struct SpectrumCarrier { double centre, bandwidth, level, floor; int32_t lo_bin, hi_bin; };
constexpr SpectrumCarrierParams kSpectrumCarrierDefaults = { 0.25, 6.0, 9, 4, 8, 0 };
// empty when acceptable, else what is wrong
std::string spectrum_carriers_check(const float* psd, int nfft, const SpectrumCarrierParams& p);
// all carriers found, sorted by centre (arguments as checked above)
std::vector<SpectrumCarrier> spectrum_carriers(const float* psd, int nfft, bool shifted, const SpectrumCarrierParams& p);

class SpectrumHip : public StreamStage {
public:
    // window: nfft floats, or null for the periodic Hann window
    SpectrumHip(int nfft, int hop, int avg, const float* window, int shifted, int max_streams, int max_samples, int device);
    // empty when the arguments are acceptable, else what is wrong with them (no device needed)
    static std::string check_args(int nfft, int hop, int avg, const float* window, int max_streams, int max_samples);
    int nfft() const { return nfft_; }
    int hop() const { return hop_; }
    int avg() const { return avg_; }
    int shifted() const { return shifted_; }
    double window_power() const { return window_power_; }
    // DEVICE pointers, d_in 8-byte and d_out 4-byte aligned, in_stride in complex elements, out_stride in floats: stream i reads n_in
    // samples at d_in + i in_stride and writes n_rows rows of nfft floats at d_out + i out_stride. Two launches at most, asynchronous
    // on `stream`, no allocation, no synchronisation. The entry (c_api_spectrum.hip) checks the arguments. One call in flight per
    // handle: the chunk sums of a call live in the handle's scratch buffer.
    int process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream);

private:
    int nfft_ = 0, log2_ = 0, hop_ = 0, avg_ = 0, shifted_ = 0;
    double window_power_ = 0.0;
    size_t scratch_floats_ = 0;
    float* d_window_ = nullptr;
    float2* d_twiddles_ = nullptr; // the table's entries in stage order, nfft - 1 of them
    float* d_scratch_ = nullptr; // chunk sums [stream][row][chunk][nfft] of the call in flight, where a row has more than one chunk
};

} // namespace dvbs2
