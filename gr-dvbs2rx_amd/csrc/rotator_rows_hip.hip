// rotator_rows_hip.hip -- see rotator_rows_hip.h.
#include "rotator_rows_hip.h"
#include "rotator_math.hpp"
#include <algorithm>
#include <cstdint>

namespace dvbs2 {

std::string rotator_rows_check(int64_t in_stride, int64_t out_stride, int n_samples, int n_streams, int64_t base_index)
{
    if (n_streams < 1 || n_streams > kRotRowsMaxStreams) return "n_streams out of range (1..65535)";
    if (n_samples < 0 || n_samples > kRotRowsMaxSamples) return "n_samples out of range (0..2^30)";
    if (n_streams > 1 && in_stride < n_samples) return "in_stride is below n_samples";
    if (n_streams > 1 && out_stride < n_samples) return "out_stride is below n_samples";
    if (base_index < 0) return "base_index is negative";
    if (base_index > INT64_MAX - n_samples) return "base_index + n_samples overflows";
    return "";
}

namespace {

constexpr int kLanes = 256;
constexpr int kMaxTiles = 4096; // workgroups along a row; a longer row is walked grid-stride, as the single-stream kernel walks its buffer

// Grid (tiles, streams). The row's record is uniform per workgroup and is loaded once; p0 is the phase of the row's first sample of this
// call, and sample i of the call has p0 + i * inc (i < 2^30: one 32 x 64 bit product, modulo 2^64). The access shape is the single-stream
// kernel's (rotator_hip.hip), decided per ROW: where the row's input and output have the same 16-byte phase, one head sample up to the
// boundary, two samples (16 bytes) per lane and step, then a tail; otherwise 8 bytes per lane and step. With an odd stride the rows
// alternate between the two phases. Every lane reads and writes its own samples only, so out == in is safe: no __restrict__ on them.
// Streaming: no LDS, no atomics; the bytes moved are those of a copy.
__global__ __launch_bounds__(kLanes) void rotator_rows_kernel(const float2* in, int64_t in_stride, float2* out, int64_t out_stride, int n,
                                                               int64_t base_index, const RotatorState* __restrict__ state)
{
    const RotatorState st = state[blockIdx.y];
    const uint64_t inc = st.inc, p0 = st.phase + ((uint64_t)base_index - (uint64_t)st.index) * inc;
    const float2* rin = in + (int64_t)blockIdx.y * in_stride;
    float2* rout = out + (int64_t)blockIdx.y * out_stride;
    const int tid = blockIdx.x * kLanes + threadIdx.x, nthreads = gridDim.x * kLanes;
    const bool vec = (((uintptr_t)rin ^ (uintptr_t)rout) & 15) == 0;
    if (!vec) {
        for (int i = tid; i < n; i += nthreads) rout[i] = rotate_one(rin[i], p0 + (uint64_t)(uint32_t)i * inc);
        return;
    }
    const int head = std::min((int)(((uintptr_t)rin >> 3) & 1), n); // one sample up to the 16-byte boundary
    const int npairs = (n - head) >> 1;
    const float4* in4 = reinterpret_cast<const float4*>(rin + head);
    float4* out4 = reinterpret_cast<float4*>(rout + head);
    for (int j = tid; j < npairs; j += nthreads) {
        const int i = head + 2 * j;
        const float4 v = in4[j];
        const float2 a = rotate_one(make_float2(v.x, v.y), p0 + (uint64_t)(uint32_t)i * inc);
        const float2 b = rotate_one(make_float2(v.z, v.w), p0 + (uint64_t)(uint32_t)(i + 1) * inc);
        out4[j] = make_float4(a.x, a.y, b.x, b.y);
    }
    if (tid == 0) {
        if (head) rout[0] = rotate_one(rin[0], p0);
        const int last = head + 2 * npairs;
        if (last < n) rout[last] = rotate_one(rin[last], p0 + (uint64_t)(uint32_t)last * inc);
    }
}

__global__ void rotator_retune_kernel(RotatorState* state, int stream_index, int64_t at_index, uint64_t inc)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    RotatorState st = state[stream_index];
    rotator_rebase(st, at_index);
    state[stream_index].phase = st.phase;
    state[stream_index].inc = inc;
    state[stream_index].index = st.index;
}

// One lane per stream; the stream's slots are walked in order and the LAST qualifying one decides (all slots of a pass were rotated by one
// increment, so their estimates are not cumulative). A stream without a qualifying slot, or whose estimate does not apply, keeps its
// 32 bytes as they are; `reserved` is never written.
__global__ __launch_bounds__(kLanes) void rotator_control_kernel(const int32_t* __restrict__ offsets, int n_streams, int max_slots,
                                                                  const float* __restrict__ coarse_foffset, const int32_t* __restrict__ coarse_corrected,
                                                                  const int32_t* __restrict__ new_est, const float* __restrict__ fine_foffset,
                                                                  const int32_t* __restrict__ fine_valid, double coarse_scale, double fine_scale,
                                                                  int64_t at_index, RotatorState* state, int32_t* applied, int64_t* delta_out)
{
    const int s = blockIdx.x * kLanes + threadIdx.x;
    if (s >= n_streams) return;
    const int a = std::max(offsets[s], 0), b = std::min(offsets[s + 1], max_slots);
    int kind = 0;
    float e = 0.0f;
    for (int i = a; i < b; i++) {
        const bool corrected = coarse_corrected[i] != 0;
        if (!corrected && new_est[i] != 0) { kind = 1; e = coarse_foffset[i]; }
        else if (corrected && fine_valid && fine_valid[i] != 0) { kind = 2; e = fine_foffset[i]; }
    }
    int64_t delta = 0;
    if (kind != 0) {
        if (rotator_adjust_turns(e, kind == 1 ? coarse_scale : fine_scale, &delta)) {
            RotatorState st = state[s];
            rotator_rebase(st, at_index);
            state[s].phase = st.phase;
            state[s].inc = st.inc - (uint64_t)delta;
            state[s].index = st.index;
        } else {
            kind = -1;
        }
    }
    if (applied) applied[s] = kind;
    if (delta_out) delta_out[s] = delta;
}

} // namespace

hipError_t rotator_rows_launch(const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int n_samples, int n_streams,
                               int64_t base_index, const RotatorState* d_state, hipStream_t stream)
{
    const int tiles = (int)std::min<int64_t>(((int64_t)n_samples / 2 + kLanes) / kLanes, kMaxTiles);
    hipLaunchKernelGGL(rotator_rows_kernel, dim3(tiles, n_streams), dim3(kLanes), 0, stream, reinterpret_cast<const float2*>(d_in), in_stride,
                       reinterpret_cast<float2*>(d_out), out_stride, n_samples, base_index, d_state);
    return hipGetLastError();
}

hipError_t rotator_retune_launch(RotatorState* d_state, int stream_index, int64_t at_index, uint64_t inc, hipStream_t stream)
{
    hipLaunchKernelGGL(rotator_retune_kernel, dim3(1), dim3(64), 0, stream, d_state, stream_index, at_index, inc);
    return hipGetLastError();
}

hipError_t rotator_control_launch(const int32_t* d_offsets, int n_streams, int max_slots, const float* d_coarse_foffset,
                                  const int32_t* d_coarse_corrected, const int32_t* d_new_est, const float* d_fine_foffset,
                                  const int32_t* d_fine_valid, double coarse_scale, double fine_scale, int64_t at_index, RotatorState* d_state,
                                  int32_t* d_applied, int64_t* d_delta, hipStream_t stream)
{
    hipLaunchKernelGGL(rotator_control_kernel, dim3((n_streams + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, d_offsets, n_streams, max_slots,
                       d_coarse_foffset, d_coarse_corrected, d_new_est, d_fine_foffset, d_fine_valid, coarse_scale, fine_scale, at_index, d_state,
                       d_applied, d_delta);
    return hipGetLastError();
}

} // namespace dvbs2
