// Micro-benchmark: issue cost of the exact instruction forms of the packed check node (check_node_v2, pair_out, two_smallest_pk) on
// gfx950, at THREE waves per SIMD (the sweep kernel's occupancy: 12 waves per CU), each with 8 independent chains per wave
// ("indep") and with one dependent chain ("dep": every instruction reads the previous one's result). Reports cycles per
// wave-instruction per SIMD at the nominal clock (wall time of the launch; 256 CUs x 3 workgroups of 4 waves).
//   hipcc --offload-arch=gfx950 -O3 -o tools/bin/node_rates tools/ubench/node_rates.hip && tools/bin/node_rates
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define ITER 8192
#define DEF(name, ASM)                                                                                                      \
    __global__ __launch_bounds__(256) void ki_##name(uint32_t* out, uint32_t seed) {                                        \
        uint32_t a0 = threadIdx.x + seed, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, a6 = a0 * 17, a7 = a0 * 19; \
        uint32_t b = seed * 77 + 5, c = seed + 9;                                                                           \
        for (int i = 0; i < ITER / 8; i++) {                                                                                \
            asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a1) : "v"(b), "v"(c));         \
            asm volatile(ASM "\n" : "+v"(a2) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a3) : "v"(b), "v"(c));         \
            asm volatile(ASM "\n" : "+v"(a4) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a5) : "v"(b), "v"(c));         \
            asm volatile(ASM "\n" : "+v"(a6) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a7) : "v"(b), "v"(c));         \
        }                                                                                                                   \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                                 \
    }                                                                                                                       \
    __global__ __launch_bounds__(256) void kd_##name(uint32_t* out, uint32_t seed) {                                        \
        uint32_t a0 = threadIdx.x + seed, b = seed * 77 + 5, c = seed + 9;                                                  \
        for (int i = 0; i < ITER / 8; i++) {                                                                                \
            asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c));         \
            asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c));         \
            asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c));         \
            asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c)); asm volatile(ASM "\n" : "+v"(a0) : "v"(b), "v"(c));         \
        }                                                                                                                   \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0;                                                                    \
    }
// full-rate references
DEF(xor_b32, "v_xor_b32 %0, %0, %1")
DEF(lshrrev_b32, "v_lshrrev_b32 %0, 8, %0")
// the forms of the packed node
DEF(pk_min_i16, "v_pk_min_i16 %0, %0, %1")
DEF(pk_max_i16, "v_pk_max_i16 %0, %0, %1")
DEF(pk_min_i16_swap, "v_pk_min_i16 %0, %0, %0 op_sel:[0,1] op_sel_hi:[1,0]")
DEF(pk_sub_i16_clamp, "v_pk_sub_i16 %0, %0, %1 clamp")
DEF(pk_add_i16_clamp, "v_pk_add_i16 %0, %0, %1 clamp")
DEF(pk_sub_i16, "v_pk_sub_i16 %0, %0, %1")
DEF(pk_ashrrev_i16, "v_pk_ashrrev_i16 %0, 15, %0")
DEF(min_u16, "v_min_u16 %0, %0, %1")
DEF(sub_u16_clamp, "v_sub_u16_e64 %0, %0, %1 clamp")
DEF(bitop3_b32, "v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96")
DEF(add3_u32, "v_add3_u32 %0, %0, %1, %2")
DEF(perm_b32, "v_perm_b32 %0, %0, %1, %2")
DEF(alignbit_b32, "v_alignbit_b32 %0, %0, %1, %2")
DEF(sub_u32_clamp, "v_sub_u32_e64 %0, %0, %1 clamp")
DEF(min3_i32, "v_min3_i32 %0, %0, %1, %2")
DEF(med3_i32, "v_med3_i32 %0, %0, %1, %2")
DEF(and_b32, "v_and_b32 %0, %0, %1")

int main() {
    uint32_t* d;
    const int blocks = 256 * 3; // 3 workgroups of 4 waves per CU -> 3 waves per SIMD
    if (hipMalloc(&d, sizeof(uint32_t) * blocks * 256) != hipSuccess) return 1;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipDeviceProp_t pr; hipGetDeviceProperties(&pr, 0);
    int khz = 0; hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, 0);
    printf("CUs %d nominal clock %d kHz, 3 waves per SIMD, %d instructions per wave\n", pr.multiProcessorCount, khz, ITER);
    printf("%-18s %12s %12s\n", "form", "indep", "dep");
    auto time = [&](void (*k)(uint32_t*, uint32_t)) {
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, d, 1u); hipDeviceSynchronize();
        float best = 1e30f;
        for (int r = 0; r < 3; r++) {
            hipEventRecord(e0); hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, d, 2u); hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
        }
        const double per_simd = (double)blocks * 4 * ITER / (pr.multiProcessorCount * 4.0); // wave-instructions per SIMD
        return best * 1e-3 * (khz * 1e3) / per_simd;
    };
#define RUN(name) printf("%-18s %12.2f %12.2f\n", #name, time(ki_##name), time(kd_##name));
    RUN(xor_b32) RUN(lshrrev_b32) RUN(and_b32) RUN(pk_min_i16) RUN(pk_max_i16) RUN(pk_min_i16_swap) RUN(pk_sub_i16_clamp) RUN(pk_add_i16_clamp)
    RUN(pk_sub_i16) RUN(pk_ashrrev_i16) RUN(min_u16) RUN(sub_u16_clamp) RUN(bitop3_b32) RUN(add3_u32) RUN(perm_b32) RUN(alignbit_b32)
    RUN(sub_u32_clamp) RUN(min3_i32) RUN(med3_i32)
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
