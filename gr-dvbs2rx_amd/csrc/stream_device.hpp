// stream_device.hpp -- what the kernels of the stream stages with a history (pulse, resamp, ddc, pfbch) have in common, and the packed
// pair every FIR of the library adds in. Device code. Internal, not installed. A stage keeps the last H samples before a call in a row
// of its history buffer: sample i of a call, i >= -H, is h[i + H] for i < 0 and the call's own sample i from 0 on.
#pragma once
#include <hip/hip_runtime.h>

namespace dvbs2 {

typedef float v2f __attribute__((ext_vector_type(2))); // (re, im): one packed multiply and one packed add per term

// Sample i of the call, -H <= i: from the row's history h0 below 0, else from the row's input x
__device__ inline float2 history_or_input(const float2* __restrict__ h0, const float2* __restrict__ x, int H, int i)
{
    return i < 0 ? h0[i + H] : x[i];
}

// Rolls one row's history h over a call of n samples, in place: afterwards h holds the last H of (old history, then the call's samples).
// fetch(j) returns sample j of the call, 0 <= j < n, as the history stores it. Every thread of the block calls it (the barrier: every
// thread reads before any thread writes), the block has kThreads threads and H <= kThreads * kPerThread; nothing is read at or past n.
template <int kThreads, int kPerThread, class Fetch> __device__ inline void roll_history(float2* __restrict__ h, int H, int n, Fetch fetch)
{
    const int t = threadIdx.x;
    float2 v[kPerThread];
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int i = t + kThreads * q;
        v[q] = make_float2(0.0f, 0.0f);
        if (i < H) {
            const long long j = (long long)i + n - H; // the sample's index in the call: below 0 it is in the old history
            v[q] = j < 0 ? h[j + H] : fetch(j);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPerThread; q++)
        if (t + kThreads * q < H) h[t + kThreads * q] = v[q];
}

} // namespace dvbs2
