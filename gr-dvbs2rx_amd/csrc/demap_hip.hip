// demap_hip.hip -- soft demapper kernels. Streaming, HBM-bound: 8 bytes in per symbol, n_mod bytes out.
//
// Arithmetic restated (all float, no FMA contraction: the file is compiled with -ffp-contract=off and the
// products below use explicit round-to-nearest intrinsics):
//   QPSK  lib/qpsk.h:208-214: scalar = (float)(2*sqrt(2) / N0); out = sat8(rint(x * scalar)) over the 2*n_syms
//         floats (volk_32f_s32f_convert_8i; VOLK is not part of the reference tree -- see oracle/demap_oracle.c).
//   8PSK  lib/psk.hh:143-150 with quantize :123-131 and rot :113; precision = (float)(4.0 / N0)
//         (lib/xfecframe_demapper_cb_impl.cc:148); column de-interleave :162-176.
//   16APSK / 32APSK  no counterpart in the reference (:70-72 throws): exact max-log over all points, demap_math.hpp and
//         notes/apsk_demap.md; natural column order, column c of a frame = label bit n_mod-1-c.
#include "demap_hip.h"
#include "demap_math.hpp"
#include <cmath>
#include "../../include/dvbs2_fec_hip.h"

namespace dvbs2 {

__global__ void demap_qpsk_kernel(const float4* __restrict__ syms, const float* __restrict__ n0, int n0_count,
                                  uint32_t* __restrict__ out, int quads_per_frame, int n_frames)
{
    const int f = blockIdx.y;
    const float N0 = n0[n0_count > 1 ? f : 0];
    const float scalar = qpsk_scalar(N0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < quads_per_frame; i += gridDim.x * blockDim.x) {
        const float4 v = syms[(size_t)f * quads_per_frame + i]; // two symbols
        const uint32_t b0 = (uint8_t)qpsk_llr(v.x, scalar), b1 = (uint8_t)qpsk_llr(v.y, scalar);
        const uint32_t b2 = (uint8_t)qpsk_llr(v.z, scalar), b3 = (uint8_t)qpsk_llr(v.w, scalar);
        out[(size_t)f * quads_per_frame + i] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
}

// One thread per FOUR consecutive symbols: two 16-byte loads, and one dword store into each of the three de-interleaved
// columns (rows = n_syms is a multiple of 4 for every frame size, so the column bases are dword aligned). One thread per
// symbol with three byte stores reached 3.9 TB/s of algorithmic bytes; a wave now stores 256 contiguous bytes per instruction.
__global__ void demap_8psk_kernel(const float4* __restrict__ syms, const float* __restrict__ n0, int n0_count,
                                  uint32_t* __restrict__ out, int n_quads, int ra0, int ra1, int ra2, float rr, float ri)
{
    const int f = blockIdx.y;
    const float N0 = n0[n0_count > 1 ? f : 0];
    const float dp = psk8_dist_prec(N0);
    uint32_t* o = out + (size_t)f * 3 * n_quads; // 3 * n_syms bytes per frame
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_quads; j += gridDim.x * blockDim.x) {
        const float4 a = syms[((size_t)f * n_quads + j) * 2], b = syms[((size_t)f * n_quads + j) * 2 + 1];
        const float re[4] = { a.x, a.z, b.x, b.z }, im[4] = { a.y, a.w, b.y, b.w };
        uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int8_t b0, b1, b2;
            psk8_llr(re[k], im[k], rr, ri, dp, b0, b1, b2);
            w0 |= (uint32_t)(uint8_t)b0 << (8 * k);
            w1 |= (uint32_t)(uint8_t)b1 << (8 * k);
            w2 |= (uint32_t)(uint8_t)b2 << (8 * k);
        }
        o[ra1 / 4 + j] = w1;
        o[ra2 / 4 + j] = w2;
        o[ra0 / 4 + j] = w0;
    }
}

// One thread per FOUR consecutive symbols, as above, and one store per column. rows = 4050 (16APSK short) is no multiple of 4: its
// odd columns start 2 bytes off a dword and its last quad holds 2 symbols. A column whose address is dword aligned gets one dword store,
// any other two 16-bit stores (a wave still writes 256 contiguous bytes); the symbols of a partial last quad are stored byte by byte.
template <int NMOD>
__global__ void __launch_bounds__(256) demap_apsk_kernel(const float* __restrict__ syms, const float* __restrict__ n0, int n0_count,
                                                         int8_t* __restrict__ out, int rows, const ApskTable t)
{
    const int f = blockIdx.y;
    const float inv_n0 = apsk_inv_n0(n0[n0_count > 1 ? f : 0]);
    const float* s = syms + (size_t)f * rows * 2;
    int8_t* o = out + (size_t)f * NMOD * rows;
    const int n_quads = (rows + 3) / 4;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += gridDim.x * blockDim.x) {
        const int j = 4 * q, n = min(4, rows - j);
        float re[4], im[4];
        if (n == 4) {
            const float4 a = reinterpret_cast<const float4*>(s)[2 * q], b = reinterpret_cast<const float4*>(s)[2 * q + 1];
            re[0] = a.x; im[0] = a.y; re[1] = a.z; im[1] = a.w; re[2] = b.x; im[2] = b.y; re[3] = b.z; im[3] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                re[k] = im[k] = 0.0f;
                if (k < n) { const float2 v = reinterpret_cast<const float2*>(s)[j + k]; re[k] = v.x; im[k] = v.y; }
            }
        }
        int8_t l[4][NMOD];
        apsk_llr2<NMOD>(t, apsk_f2{ re[0], re[1] }, apsk_f2{ im[0], im[1] }, inv_n0, l[0], l[1]);
        apsk_llr2<NMOD>(t, apsk_f2{ re[2], re[3] }, apsk_f2{ im[2], im[3] }, inv_n0, l[2], l[3]);
#pragma unroll
        for (int c = 0; c < NMOD; c++) {
            int8_t* col = o + (size_t)c * rows; // the same for every thread of the block: the choice of store width is a scalar branch
            int8_t* p = col + j;
            const uint32_t w = (uint32_t)(uint8_t)l[0][c] | ((uint32_t)(uint8_t)l[1][c] << 8) | ((uint32_t)(uint8_t)l[2][c] << 16) | ((uint32_t)(uint8_t)l[3][c] << 24);
            if (n == 4 && ((uintptr_t)col & 3) == 0) *reinterpret_cast<uint32_t*>(p) = w;
            else if (n == 4 && ((uintptr_t)col & 1) == 0) {
                reinterpret_cast<uint16_t*>(p)[0] = (uint16_t)w; reinterpret_cast<uint16_t*>(p)[1] = (uint16_t)(w >> 16);
            } else
                for (int k = 0; k < n; k++) p[k] = (int8_t)(w >> (8 * k));
        }
    }
}

// One workgroup per frame. llr == nullptr: reference point = hard slice of the symbol (pre-decoder estimate);
// otherwise the reference point is re-mapped from the signs of the decoded LLRs (post-decoder refinement,
// lib/xfecframe_demapper_cb_impl.cc:268-307, lib/qpsk.h:266-281): LLR < 0 -> -1, else +1; 8PSK bits are picked
// through the column interleaver (ra0..2 = d_rowaddr0..2).
__global__ void demap_snr_kernel(const float2* __restrict__ syms, const int8_t* __restrict__ llr, float* __restrict__ snr,
                                 int n_syms, int constellation, int ra0, int ra1, int ra2, float rr, float ri)
{
    __shared__ float ssp[256], snp[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float rs2 = 0.70710678118654752440f;
    float sp = 0, np = 0;
    for (int j = tid; j < n_syms; j += blockDim.x) {
        const float2 c = syms[(size_t)f * n_syms + j];
        float sr, si;
        if (constellation == DVBS2_MOD_QPSK) {
            if (llr) {
                const int8_t* l = llr + (size_t)f * 2 * n_syms + 2 * j;
                sr = l[0] >= 0 ? rs2 : -rs2; si = l[1] >= 0 ? rs2 : -rs2;
            } else { sr = c.x >= 0 ? rs2 : -rs2; si = c.y >= 0 ? rs2 : -rs2; }
        } else {
            int b0, b1, b2;
            if (llr) {
                const int8_t* l = llr + (size_t)f * 3 * n_syms;
                b0 = l[ra0 + j] < 0 ? -1 : 1; b1 = l[ra1 + j] < 0 ? -1 : 1; b2 = l[ra2 + j] < 0 ? -1 : 1;
            } else {
                const float cr = c.x * rr - c.y * ri, ci = c.x * ri + c.y * rr;
                b1 = cr < 0 ? -1 : 1; b2 = ci < 0 ? -1 : 1; b0 = fabsf(cr) < fabsf(ci) ? -1 : 1;
            }
            const int idx = (((b0 + 1) << 1) ^ 0x4) | ((b1 + 1) ^ 0x2) | (((b2 + 1) >> 1) ^ 0x1);
            const float m8r[8] = { rs2, 1, -1, -rs2, 0, rs2, -rs2, 0 }, m8i[8] = { rs2, 0, 0, -rs2, 1, -rs2, rs2, -1 };
            sr = m8r[idx]; si = m8i[idx];
        }
        const float er = c.x - sr, ei = c.y - si;
        sp += sr * sr + si * si; np += er * er + ei * ei;
    }
    snr_block_reduce(sp, np, ssp, snp, snr + f);
}

// The same for 16APSK / 32APSK. llr == nullptr: the reference point is the nearest of all points (the lowest label on a tie);
// otherwise its label is read from the signs of the decoded LLRs, column c = label bit NMOD-1-c.
template <int NMOD>
__global__ void demap_snr_apsk_kernel(const float2* __restrict__ syms, const int8_t* __restrict__ llr, float* __restrict__ snr,
                                      int n_syms, const ApskTable t)
{
    __shared__ float ssp[256], snp[256];
    constexpr int M = 1 << NMOD;
    const int f = blockIdx.x;
    float sp = 0, np = 0;
    for (int j = threadIdx.x; j < n_syms; j += blockDim.x) {
        const float2 c = syms[(size_t)f * n_syms + j];
        float sr = t.re[0], si = t.im[0];
        if (llr) {
            const int8_t* l = llr + (size_t)f * NMOD * n_syms + j;
            int label = 0;
#pragma unroll
            for (int k = 0; k < NMOD; k++) label |= (l[(size_t)k * n_syms] < 0 ? 1 : 0) << (NMOD - 1 - k);
#pragma unroll
            for (int i = 1; i < M; i++) if (label == i) { sr = t.re[i]; si = t.im[i]; }
        } else {
            float best = 0;
#pragma unroll
            for (int i = 0; i < M; i++) {
                const float dr = c.x - t.re[i], di = c.y - t.im[i], d = dr * dr + di * di;
                if (i == 0 || d < best) { best = d; sr = t.re[i]; si = t.im[i]; }
            }
        }
        const float er = c.x - sr, ei = c.y - si;
        sp += sr * sr + si * si; np += er * er + ei * ei;
    }
    snr_block_reduce(sp, np, ssp, snp, snr + f);
}

// EN 302 307-1 5.4.3 / 5.4.4, Es = 1. Restated from the standard; the reference has neither a modulator nor a demapper for these.
bool apsk_points(int constellation, int rate, float* re_im)
{
    // rate enumerators (dvb_config.h:20-72): C2_3 = 5, C3_4 = 6, C4_5 = 7, C5_6 = 8, C8_9 = 10, C9_10 = 11
    static const double g16[12] = { 0, 0, 0, 0, 0, 3.15, 2.85, 2.75, 2.70, 0, 2.60, 2.57 };
    static const double g32a[12] = { 0, 0, 0, 0, 0, 0, 2.84, 2.72, 2.64, 0, 2.54, 2.53 };
    static const double g32b[12] = { 0, 0, 0, 0, 0, 0, 5.27, 4.87, 4.64, 0, 4.33, 4.30 };
    if (rate < 0 || rate > 11) return false;
    if (constellation == DVBS2_MOD_16APSK) {
        const double g = g16[rate];
        if (g == 0) return false;
        const double r1 = 2.0 / std::sqrt(1.0 + 3.0 * g * g), r2 = g * r1;
        static const int ang[16] = { 3, -3, 9, -9, 1, -1, 11, -11, 5, -5, 7, -7, 3, -3, 9, -9 }; // units of pi/12
        for (int i = 0; i < 16; i++) {
            const double r = i < 12 ? r2 : r1, a = ang[i] * (M_PI / 12);
            re_im[2 * i] = (float)(r * std::cos(a)); re_im[2 * i + 1] = (float)(r * std::sin(a));
        }
        return true;
    }
    if (constellation == DVBS2_MOD_32APSK) {
        const double g1 = g32a[rate], g2 = g32b[rate];
        if (g1 == 0) return false;
        const double r1 = std::sqrt(32.0 / (4.0 + 12.0 * g1 * g1 + 16.0 * g2 * g2)), r[3] = { r1, g1 * r1, g2 * r1 };
        static const int ang[32] = { 6, 10, -6, -10, 18, 14, -18, -14, 3, 9, -6, -12, 18, 12, -21, -15,
                                     2, 6, -2, -6, 22, 18, -22, -18, 0, 6, -3, -9, 21, 15, 24, -18 }; // units of pi/24
        static const int ring[32] = { 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 1, 0, 1, 0, 1, 0, 1, 0, 2, 2, 2, 2, 2, 2, 2, 2 };
        for (int i = 0; i < 32; i++) {
            const double a = ang[i] * (M_PI / 24);
            re_im[2 * i] = (float)(r[ring[i]] * std::cos(a)); re_im[2 * i + 1] = (float)(r[ring[i]] * std::sin(a));
        }
        return true;
    }
    return false;
}

DemapperHip::DemapperHip(int framesize, int rate, int constellation, int max_frames, int device)
    : DeviceStage(device), constellation_(constellation), max_frames_(max_frames)
{
    n_llr_ = framesize == DVBS2_FECFRAME_NORMAL ? 64800 : framesize == DVBS2_FECFRAME_MEDIUM ? 32400 : 16200;
    if (constellation == DVBS2_MOD_QPSK) n_mod_ = 2;
    else if (constellation == DVBS2_MOD_8PSK) {
        n_mod_ = 3;
        // rate enumerators: C3_5 = 4; C25_36 = 26, C13_18 = 28, C7_15 = 38, C8_15 = 39, C26_45 = 19 (dvb_config.h:20-72)
        if (rate == 4) order_ = 1;                                                              // "210"
        else if (rate == 26 || rate == 28 || rate == 38 || rate == 39 || rate == 19) order_ = 2; // "102"
        else order_ = 0;                                                                         // "012"
    } else if (constellation == DVBS2_MOD_16APSK || constellation == DVBS2_MOD_32APSK) {
        n_mod_ = constellation == DVBS2_MOD_16APSK ? 4 : 5;
        float p[64];
        if (framesize == DVBS2_FECFRAME_MEDIUM) { err_.argument("Unsupported frame size for 16APSK / 32APSK (normal and short only)"); return; }
        if (!apsk_points(constellation, rate, p) || (rate == 11 && framesize != DVBS2_FECFRAME_NORMAL)) {
            err_.argument("Unsupported code rate for 16APSK / 32APSK (DVB-S2: 16APSK 2/3 .. 9/10, 32APSK 3/4 .. 9/10; 9/10 normal frames only)"); return;
        }
        for (int i = 0; i < (1 << n_mod_); i++) { apsk_.re[i] = p[2 * i]; apsk_.im[i] = p[2 * i + 1]; }
    } else { err_.argument("Unsupported constellation"); return; }
    if (max_frames_ < 1 || max_frames_ > 65535) { err_.argument("max_frames must be in 1..65535 (frames are one launch dimension)"); return; }
}

int DemapperHip::soft_device(const float* d_syms, int n_frames, const float* d_n0, int n0_count, int8_t* d_llr, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames == 0) return 0;
    if (constellation_ == DVBS2_MOD_QPSK) {
        const int quads = n_llr_ / 4;
        hipLaunchKernelGGL(demap_qpsk_kernel, dim3((quads + 255) / 256, n_frames), dim3(256), 0, stream,
                           reinterpret_cast<const float4*>(d_syms), d_n0, n0_count, reinterpret_cast<uint32_t*>(d_llr), quads, n_frames);
    } else if (table_ && !table_as_apsk_) launch_table(d_syms, n_frames, d_n0, n0_count, d_llr, stream);
    else if (is_apsk() || table_as_apsk_) {
        const int rows = n_syms(), quads = (rows + 3) / 4; // 16200 / 4050 (16APSK), 12960 / 3240 (32APSK)
        const dim3 grid((quads + 255) / 256, n_frames);
        if (n_mod_ == 4) hipLaunchKernelGGL(demap_apsk_kernel<4>, grid, dim3(256), 0, stream, d_syms, d_n0, n0_count, d_llr, rows, apsk_);
        else hipLaunchKernelGGL(demap_apsk_kernel<5>, grid, dim3(256), 0, stream, d_syms, d_n0, n0_count, d_llr, rows, apsk_);
    } else {
        const int rows = n_syms();
        int ra0 = 0, ra1 = rows, ra2 = 2 * rows;
        if (order_ == 1) { ra0 = 2 * rows; ra1 = rows; ra2 = 0; }
        else if (order_ == 2) { ra0 = rows; ra1 = 0; ra2 = 2 * rows; }
        const float rr = (float)std::cos(-M_PI / 8), ri = (float)std::sin(-M_PI / 8); // (complexf) exp(-j pi/8)
        const int quads = rows / 4; // 21600, 10800, 5400 symbols: a multiple of 4
        hipLaunchKernelGGL(demap_8psk_kernel, dim3((quads + 255) / 256, n_frames), dim3(256), 0, stream,
                           reinterpret_cast<const float4*>(d_syms), d_n0, n0_count, reinterpret_cast<uint32_t*>(d_llr), quads, ra0, ra1, ra2, rr, ri);
    }
    return launched("demap kernel launch");
}

DemapFused DemapperHip::fused(const float* d_syms, const float* d_n0, int n0_count) const
{
    DemapFused d{};
    d.syms = d_syms; d.n0 = d_n0; d.n0_count = n0_count; d.n_syms = n_syms();
    d.mode = constellation_ == DVBS2_MOD_QPSK ? 1 : 2;
    const int rows = n_syms();
    d.ra0 = 0; d.ra1 = rows; d.ra2 = 2 * rows;
    if (order_ == 1) { d.ra0 = 2 * rows; d.ra1 = rows; d.ra2 = 0; }
    else if (order_ == 2) { d.ra0 = rows; d.ra1 = 0; d.ra2 = 2 * rows; }
    d.rr = (float)std::cos(-M_PI / 8); d.ri = (float)std::sin(-M_PI / 8);
    return d;
}

int DemapperHip::snr_device(const float* d_syms, const int8_t* d_ref_llr, int n_frames, float* d_snr, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames == 0) return 0;
    const float rr = (float)std::cos(-M_PI / 8), ri = (float)std::sin(-M_PI / 8);
    const int rows = n_syms();
    int ra0 = 0, ra1 = rows, ra2 = 2 * rows;
    if (order_ == 1) { ra0 = 2 * rows; ra1 = rows; ra2 = 0; }
    else if (order_ == 2) { ra0 = rows; ra1 = 0; ra2 = 2 * rows; }
    if (table_) launch_table_snr(d_syms, d_ref_llr, n_frames, d_snr, stream);
    else if (is_apsk() && n_mod_ == 4)
        hipLaunchKernelGGL(demap_snr_apsk_kernel<4>, dim3(n_frames), dim3(256), 0, stream, reinterpret_cast<const float2*>(d_syms), d_ref_llr, d_snr, rows, apsk_);
    else if (is_apsk())
        hipLaunchKernelGGL(demap_snr_apsk_kernel<5>, dim3(n_frames), dim3(256), 0, stream, reinterpret_cast<const float2*>(d_syms), d_ref_llr, d_snr, rows, apsk_);
    else
        hipLaunchKernelGGL(demap_snr_kernel, dim3(n_frames), dim3(256), 0, stream,
                           reinterpret_cast<const float2*>(d_syms), d_ref_llr, d_snr, rows, constellation_, ra0, ra1, ra2, rr, ri);
    return launched("snr kernel launch");
}

} // namespace dvbs2
