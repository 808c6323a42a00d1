// rotator_math.hpp -- the one sample of the rotator (rotator_hip.h): x e^{j phi} from the 64-bit fixed-point phase `ph` in turns. Shared by
// the kernels that mix with the rotator's arithmetic (rotator_hip.hip, ddc_hip.hip), so that they agree bit for bit. Device code only;
// the translation unit is built without contraction (-ffp-contract=off): four products, a subtraction and an addition.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dvbs2 {

__device__ inline float2 rotate_one(float2 x, uint64_t ph)
{
    const float t = (float)(int32_t)(uint32_t)(ph >> 32) * 0x1p-31f; // half-turns in [-1, 1]
    float s, c;
    sincospif(t, &s, &c);
    return make_float2(x.x * c - x.y * s, x.x * s + x.y * c);
}

} // namespace dvbs2
