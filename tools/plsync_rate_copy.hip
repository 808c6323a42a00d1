// plsync_rate_copy.hip -- the comparison partner of tools/plsync_rate.py: a hand-written device-to-device copy with 16-byte
// accesses, one float4 per thread and grid step. Built by the tool into tools/bin/.
#include <hip/hip_runtime.h>
#include <cstddef>

__global__ __launch_bounds__(256) void copy16_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n16)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += step) dst[i] = src[i];
}

// n16 float4 values from src to dst on `stream`; returns the HIP error code of the launch
extern "C" int plsync_rate_copy16(void* dst, const void* src, size_t n16, void* stream)
{
    const size_t want = (n16 + 255) / 256;
    const unsigned blocks = (unsigned)(want < 256u * 32u ? (want ? want : 1) : 256u * 32u); // 32 workgroups per CU at most
    hipLaunchKernelGGL(copy16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)src, (float4*)dst, n16);
    return (int)hipGetLastError();
}
