// rotator_rows_hip.h -- the rotator for a batch of streams from state held in DEVICE memory, and the frequency-control step that steers
// it from the per-slot PL estimates (include/dvbs2_fec_hip.h, "rotator rows"; notes/rotator_rows.md).
//   A stream's state is one 32-byte record in the caller's device memory: the phase in turns (2^64 = one turn) AT an absolute sample
//   index, and the increment in turns per sample. Sample m has the phase  phase + (m - index) * inc  modulo 2^64, for any m: the rotation
//   only READS the record, so a rotated sample is a pure function of (record, absolute index) -- as a noise sample of awgn_hip.h is of
//   (seed, stream, index). Pieces equal one call, a block can be replayed, any number of calls may be in flight. The sample itself is
//   rotate_one of rotator_math.hpp, unchanged: a row started by rotator_inc_turns(inc) at phase 0, index 0 is a RotatorHip(inc), bit for bit.
//   An increment changes by REBASING the record at an absolute index: phase += (at - index) * inc; index = at; inc = new. The phase stays
//   continuous across the change. The retune kernel does that with a given increment, the control kernel with  inc -= delta  where delta
//   comes from the last qualifying estimate of the stream's slots (rule: the header).
// There is no handle, no allocation and no host synchronisation here; the three launches are asynchronous on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

namespace dvbs2 {

struct RotatorState { uint64_t phase, inc; int64_t index; uint64_t reserved; }; // dvbs2_rotator_state_t

// The ONE conversion of the control step, the same arithmetic on the host and on the device: d = estimate * scale in double (one
// product; the unit is built without contraction), applies = d finite and |d| < 0.5 turns per sample, delta = d * 2^64 (exact) rounded
// to nearest even -- it fits int64 because |d| < 0.5. Without `applies` delta is 0.
__host__ __device__ inline bool rotator_adjust_turns(float estimate, double scale, int64_t* delta)
{
    const double d = (double)estimate * scale;
    const bool applies = d - d == 0.0 && fabs(d) < 0.5;
    *delta = applies ? (int64_t)llrint(d * 0x1p64) : 0;
    return applies;
}

// the record seen from absolute index `at`: the same phase function, written from there
__host__ __device__ inline void rotator_rebase(RotatorState& st, int64_t at)
{
    st.phase += ((uint64_t)at - (uint64_t)st.index) * st.inc;
    st.index = at;
}

constexpr int kRotRowsMaxStreams = 65535;  // the y extent of a grid
constexpr int kRotRowsMaxSamples = 1 << 30;

// "" or what is wrong, naming the argument; strides matter only with n_streams > 1
std::string rotator_rows_check(int64_t in_stride, int64_t out_stride, int n_samples, int n_streams, int64_t base_index);

// One launch each on `stream` of the current device; the hipError_t of the launch. Arguments are the C entry's, already checked.
hipError_t rotator_rows_launch(const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int n_samples, int n_streams,
                               int64_t base_index, const RotatorState* d_state, hipStream_t stream);
hipError_t rotator_retune_launch(RotatorState* d_state, int stream_index, int64_t at_index, uint64_t inc, hipStream_t stream);
hipError_t rotator_control_launch(const int32_t* d_offsets, int n_streams, int max_slots, const float* d_coarse_foffset,
                                  const int32_t* d_coarse_corrected, const int32_t* d_new_est, const float* d_fine_foffset,
                                  const int32_t* d_fine_valid, double coarse_scale, double fine_scale, int64_t at_index, RotatorState* d_state,
                                  int32_t* d_applied, int64_t* d_delta, hipStream_t stream);

} // namespace dvbs2
