// demap_math.hpp -- the soft-demapper arithmetic as device functions, shared by the stand-alone demapper kernels (demap_hip.hip)
// and by the LDPC sweep kernels, which can take XFECFRAME symbols directly and demap while they load a frame into LDS
// (one launch and 2 N bytes of HBM traffic per frame less than demapper -> LLR buffer -> decoder).
// Arithmetic restated (all float, no FMA contraction: compiled with -ffp-contract=off, products by explicit round-to-nearest
// intrinsics):
//   QPSK  lib/qpsk.h:208-214: scalar = (float)(2*sqrt(2) / N0); out = sat8(rint(x * scalar)) (volk_32f_s32f_convert_8i; VOLK is
//         not part of the reference tree -- see oracle/demap_oracle.c).
//   8PSK  lib/psk.hh:143-150 with quantize :123-131 and rot :113; precision = (float)(4.0 / N0)
//         (lib/xfecframe_demapper_cb_impl.cc:148); column de-interleave :162-176.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dvbs2 {

__device__ __forceinline__ int8_t sat8_rint(float v)
{
    if (v > 127.0f) return 127;
    if (v < -128.0f) return -128;
    return (int8_t)rintf(v);
}
__device__ __forceinline__ float qpsk_scalar(float N0) { return (float)(2.0 * 1.41421356237309504880 / (double)N0); }
__device__ __forceinline__ int8_t qpsk_llr(float x, float scalar) { return sat8_rint(__fmul_rn(x, scalar)); }

__device__ __forceinline__ int8_t quant8(float dist_prec, float value)
{
    value = __fmul_rn(value, dist_prec);
    value = rintf(value);
    value = fminf(fmaxf(value, -128.0f), 127.0f);
    return (int8_t)value;
}
__device__ __forceinline__ float psk8_dist_prec(float N0)
{
    const float precision = (float)(4.0 / (double)N0);
    const float sin_pi_8 = 0.38268343236508977173f;
    return __fmul_rn(2 * sin_pi_8, precision);
}
// the three LLRs of one 8PSK symbol in the order soft[0], soft[1], soft[2] of PhaseShiftKeying<8>::soft
__device__ __forceinline__ void psk8_llr(float re, float im, float rr, float ri, float dp, int8_t& b0, int8_t& b1, int8_t& b2)
{
    const float rcp_sqrt_2 = 0.70710678118654752440f;
    const float cr = __fsub_rn(__fmul_rn(re, rr), __fmul_rn(im, ri));
    const float ci = __fadd_rn(__fmul_rn(re, ri), __fmul_rn(im, rr));
    b1 = quant8(dp, cr);
    b2 = quant8(dp, ci);
    b0 = quant8(dp, __fmul_rn(rcp_sqrt_2, __fsub_rn(fabsf(cr), fabsf(ci))));
}

// 16APSK / 32APSK (EN 302 307-1 5.4.3 / 5.4.4; no counterpart in the reference, notes/apsk_demap.md): exact max-log over ALL M = 2^NMOD
// points, L_b = (min_{s: bit b = 1} |y - s|^2 - min_{s: bit b = 0} |y - s|^2) / N0 in natural-log units (QPSK's scale).
// The table travels as a kernel argument: every index below is a compile-time constant after unrolling, so the points stay in SGPRs.
struct ApskTable {
    float re[32], im[32]; // entry i = the point whose label is i; label bit NMOD-1 (the most significant) is the first interleaver column
};
typedef float apsk_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float apsk_inv_n0(float N0) { return (float)(1.0 / (double)N0); }
// Two symbols at once (re = {re_a, re_b}, im likewise): the subtractions, products and the sum are element-wise IEEE operations (no
// contraction), which the compiler may issue as v_pk_add_f32 / v_pk_mul_f32; the minima are scalar. llr[c] = column c = label bit NMOD-1-c.
template <int NMOD>
__device__ __forceinline__ void apsk_llr2(const ApskTable& t, apsk_f2 re, apsk_f2 im, float inv_n0, int8_t (&la)[NMOD], int8_t (&lb)[NMOD])
{
#pragma clang fp contract(off)
    constexpr int M = 1 << NMOD;
    float m0a[NMOD], m1a[NMOD], m0b[NMOD], m1b[NMOD];
#pragma unroll
    for (int i = 0; i < M; i++) {
        const apsk_f2 dr = re - t.re[i], di = im - t.im[i];
        const apsk_f2 d = dr * dr + di * di;
#pragma unroll
        for (int c = 0; c < NMOD; c++) {
            const int bit = 1 << (NMOD - 1 - c);
            if (i == 0) { m0a[c] = d.x; m0b[c] = d.y; }           // the first point with a 0 in column c
            else if (i == bit) { m1a[c] = d.x; m1b[c] = d.y; }    // the first with a 1
            else if (i & bit) { m1a[c] = fminf(m1a[c], d.x); m1b[c] = fminf(m1b[c], d.y); }
            else { m0a[c] = fminf(m0a[c], d.x); m0b[c] = fminf(m0b[c], d.y); }
        }
    }
#pragma unroll
    for (int c = 0; c < NMOD; c++) {
        la[c] = sat8_rint(__fmul_rn(__fsub_rn(m1a[c], m0a[c]), inv_n0));
        lb[c] = sat8_rint(__fmul_rn(__fsub_rn(m1b[c], m0b[c]), inv_n0));
    }
}

// the tail of every SNR kernel (demap_hip.hip, demap_table_hip.hip): block sum of the two powers, snr = signal / noise
__device__ __forceinline__ void snr_block_reduce(float sp, float np, float* ssp, float* snp, float* snr)
{
    const int tid = threadIdx.x;
    ssp[tid] = sp; snp[tid] = np;
    __syncthreads();
    for (int s = 128; s; s >>= 1) { if (tid < s) { ssp[tid] += ssp[tid + s]; snp[tid] += snp[tid + s]; } __syncthreads(); }
    if (tid == 0) { float n = snp[0]; if (!(n > 0)) n = 1e-12f; *snr = ssp[0] / n; }
}

// What a sweep kernel needs to demap while loading (passed by value; mode 0 = LLR input)
struct DemapFused {
    const float* syms;  // n_frames * n_syms complex symbols (re, im)
    const float* n0;    // one value, or one per frame
    int n0_count;
    int mode;           // 0 none, 1 QPSK, 2 8PSK
    int n_syms;
    int ra0, ra1, ra2;  // 8PSK column bases (d_rowaddr0..2)
    float rr, ri;       // (complexf) exp(-j pi/8)
};

} // namespace dvbs2
