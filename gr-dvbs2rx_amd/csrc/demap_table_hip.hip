// demap_table_hip.hip -- soft demapping of a CALLER's constellation table of 4 .. 256 labelled points (dvbs2_demap_create_table):
// the exact max-log LLR of demap_math.hpp / notes/apsk_demap.md over all 2^n_mod points, the caller's column order, and the two SNR
// estimates. Kernel form, forms considered, register counts and rates: notes/demap_table.md.
//
// Arithmetic (all float, one correctly rounded operation each, no contraction: -ffp-contract=off and the pragma below):
//   dr = re - p.re; di = im - p.im; d = dr * dr + di * di                      for all 2^n_mod points
//   L_b = (min_{label bit b = 1} d - min_{label bit b = 0} d) * (float)(1.0 / (double)N0);  llr = sat8(rint(L_b))
// A float minimum is exact, so the tree below gives the bits of the label-order loop of tests/apsk_model.py::demap_f32.
#include "demap_hip.h"
#include "demap_math.hpp"
#include <cmath>
#include <cstring>
#include "../../include/dvbs2_fec_hip.h"

namespace dvbs2 {

// Label i = (u << LO) | l with LO = ceil(NMOD / 2) low bits. Per symbol: the minimum over the row u (all l) goes into the minima of
// the HI upper bits as soon as the row is done, the minima over the columns l (all u) are kept (2^LO registers) and give the minima
// of the LO lower bits at the end: 2 minima per point and symbol instead of NMOD.
// One thread per FOUR consecutive symbols (two 2-vectors, as apsk_llr2): one 16-byte LDS read -- the same address in every lane, a
// broadcast -- brings two points and feeds eight distances. Stores as demap_apsk_kernel: one per column and thread, the width by
// the column's byte address (a scalar branch), a partial last quad byte by byte. pos: byte b = the column of label bit b (0 = MSB).
template <int NMOD>
__global__ void __launch_bounds__(256) demap_table_kernel(const float* __restrict__ syms, const float* __restrict__ n0, int n0_count,
                                                          int8_t* __restrict__ out, int rows, const float4* __restrict__ table, const uint64_t pos)
{
#pragma clang fp contract(off)
    constexpr int M = 1 << NMOD, LO = (NMOD + 1) / 2, HI = NMOD - LO, L = 1 << LO, U = 1 << HI;
    constexpr uint32_t kInf = 0x7f800000u; // +infinity
    constexpr int UNROLL_U = NMOD >= 6 ? 4 : NMOD >= 4 ? 1 : U; // the row loop stays a loop from 16 points on: unrolled, 32 points take all 256 VGPRs
    __shared__ float4 tab[M / 2]; // (re, im) of label 2 i and of label 2 i + 1
    if (threadIdx.x < M / 2) tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int f = blockIdx.y;
    const float inv_n0 = apsk_inv_n0(n0[n0_count > 1 ? f : 0]);
    const float* s = syms + (size_t)f * rows * 2;
    int8_t* o = out + (size_t)f * NMOD * rows;
    const int n_quads = (rows + 3) / 4;
    const bool wide = ((uintptr_t)s & 15) == 0; // an odd n_syms puts every other frame 8 bytes off
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += gridDim.x * blockDim.x) {
        const int j = 4 * q, n = min(4, rows - j);
        apsk_f2 re[2], im[2];
        if (n == 4 && wide) {
            const float4 a = reinterpret_cast<const float4*>(s)[2 * q], b = reinterpret_cast<const float4*>(s)[2 * q + 1];
            re[0] = apsk_f2{ a.x, a.z }; im[0] = apsk_f2{ a.y, a.w }; re[1] = apsk_f2{ b.x, b.z }; im[1] = apsk_f2{ b.y, b.w };
        } else {
            float r[4], i[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                r[k] = i[k] = 0.0f;
                if (k < n) { const float2 v = reinterpret_cast<const float2*>(s)[j + k]; r[k] = v.x; i[k] = v.y; }
            }
            re[0] = apsk_f2{ r[0], r[1] }; im[0] = apsk_f2{ i[0], i[1] }; re[1] = apsk_f2{ r[2], r[3] }; im[1] = apsk_f2{ i[2], i[3] };
        }
        // The minima are taken on the BIT PATTERNS as unsigned integers: a squared distance is +0 or larger, never -0, and among such
        // floats the integer order is the float order, so the result is the float minimum bit for bit. It spares the instruction
        // that quiets a possible signalling NaN in front of every float minimum on a value carried around the row loop.
        uint32_t colmin[4][L], m0[4][NMOD], m1[4][NMOD]; // m0 / m1 by label bit, 0 = most significant
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int l = 0; l < L; l++) colmin[k][l] = kInf;
#pragma unroll
            for (int b = 0; b < NMOD; b++) m0[k][b] = m1[k][b] = kInf;
        }
#pragma unroll UNROLL_U
        for (int u = 0; u < U; u++) {
            uint32_t rowmin[4] = { kInf, kInf, kInf, kInf };
#pragma unroll
            for (int l = 0; l < L; l += 2) {
                const float4 p = tab[(u * L + l) / 2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const apsk_f2 dra = re[h] - p.x, dia = im[h] - p.y, drb = re[h] - p.z, dib = im[h] - p.w;
                    const apsk_f2 da = dra * dra + dia * dia, db = drb * drb + dib * dib;
                    const uint32_t ax = __float_as_uint(da.x), ay = __float_as_uint(da.y), bx = __float_as_uint(db.x), by = __float_as_uint(db.y);
                    rowmin[2 * h] = min(min(rowmin[2 * h], ax), bx);
                    rowmin[2 * h + 1] = min(min(rowmin[2 * h + 1], ay), by);
                    colmin[2 * h][l] = min(colmin[2 * h][l], ax); colmin[2 * h + 1][l] = min(colmin[2 * h + 1][l], ay);
                    colmin[2 * h][l + 1] = min(colmin[2 * h][l + 1], bx); colmin[2 * h + 1][l + 1] = min(colmin[2 * h + 1][l + 1], by);
                }
            }
#pragma unroll
            for (int b = 0; b < HI; b++) {
                const bool one = (u >> (HI - 1 - b)) & 1; // the same in every lane
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (one) m1[k][b] = min(m1[k][b], rowmin[k]);
                    else m0[k][b] = min(m0[k][b], rowmin[k]);
                }
            }
        }
#pragma unroll
        for (int b = HI; b < NMOD; b++) {
#pragma unroll
            for (int l = 0; l < L; l++) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if ((l >> (NMOD - 1 - b)) & 1) m1[k][b] = min(m1[k][b], colmin[k][l]);
                    else m0[k][b] = min(m0[k][b], colmin[k][l]);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < NMOD; b++) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) w |= (uint32_t)(uint8_t)sat8_rint(__fmul_rn(__fsub_rn(__uint_as_float(m1[k][b]), __uint_as_float(m0[k][b])), inv_n0)) << (8 * k);
            int8_t* col = o + (size_t)((pos >> (8 * b)) & 0xff) * rows; // the same for every thread of the block
            int8_t* p = col + j;
            if (n == 4 && ((uintptr_t)col & 3) == 0) *reinterpret_cast<uint32_t*>(p) = w;
            else if (n == 4 && ((uintptr_t)col & 1) == 0) {
                reinterpret_cast<uint16_t*>(p)[0] = (uint16_t)w; reinterpret_cast<uint16_t*>(p)[1] = (uint16_t)(w >> 16);
            } else
                for (int k = 0; k < n; k++) p[k] = (int8_t)(w >> (8 * k));
        }
    }
}

// One workgroup per frame, the table in LDS. llr == nullptr: the reference point is the nearest of all points (the lowest label on a
// tie); otherwise its label is spelled by the signs of the decoded LLRs: label bit column[c] (0 = MSB) of symbol j is
// llr[c * n_syms + j] < 0. cols: byte c = column[c].
__global__ void __launch_bounds__(256) demap_snr_table_kernel(const float2* __restrict__ syms, const int8_t* __restrict__ llr, float* __restrict__ snr,
                                                              int n_syms, int n_mod, const float2* __restrict__ table, const uint64_t cols)
{
    __shared__ float ssp[256], snp[256];
    __shared__ float2 tab[256];
    const int f = blockIdx.x, M = 1 << n_mod;
    for (int i = threadIdx.x; i < M; i += blockDim.x) tab[i] = table[i];
    __syncthreads();
    float sp = 0, np = 0;
    for (int j = threadIdx.x; j < n_syms; j += blockDim.x) {
        const float2 c = syms[(size_t)f * n_syms + j];
        int label = 0;
        if (llr) {
            const int8_t* l = llr + (size_t)f * n_mod * n_syms + j;
            for (int k = 0; k < n_mod; k++) label |= (l[(size_t)k * n_syms] < 0 ? 1 : 0) << (n_mod - 1 - (int)((cols >> (8 * k)) & 0xff));
        } else {
            float best = 0;
            for (int i = 0; i < M; i++) {
                const float2 p = tab[i];
                const float dr = c.x - p.x, di = c.y - p.y, d = dr * dr + di * di;
                if (i == 0 || d < best) { best = d; label = i; }
            }
        }
        const float2 r = tab[label];
        const float er = c.x - r.x, ei = c.y - r.y;
        sp += r.x * r.x + r.y * r.y; np += er * er + ei * ei;
    }
    snr_block_reduce(sp, np, ssp, snp, snr + f);
}

// The one place that judges a caller's table (dvbs2_demap_table_check and the constructor below). Host only.
bool demap_table_check(int n_mod, const float* points_re_im, const uint8_t* column, std::string* why)
{
    std::string w;
    if (n_mod == 7) w = "n_mod 7 is not supported: no DVB frame length (16200, 32400, 64800) is a multiple of 7";
    else if (n_mod != 2 && n_mod != 3 && n_mod != 4 && n_mod != 5 && n_mod != 6 && n_mod != 8)
        w = "n_mod must be one of 2, 3, 4, 5, 6, 8 (a table of 4 .. 256 points), not " + std::to_string(n_mod);
    else if (!points_re_im) w = "points_re_im is NULL";
    else {
        for (int i = 0; i < (2 << n_mod) && w.empty(); i++)
            if (!std::isfinite(points_re_im[i]))
                w = "points_re_im: the " + std::string(i & 1 ? "imaginary" : "real") + " part of point " + std::to_string(i / 2) + " is not finite";
        if (w.empty() && column) {
            unsigned seen = 0;
            for (int c = 0; c < n_mod && w.empty(); c++) {
                if (column[c] >= n_mod) w = "column[" + std::to_string(c) + "] = " + std::to_string(column[c]) + " is out of range 0 .. n_mod-1";
                else if (seen & (1u << column[c])) w = "column is not a permutation of 0 .. n_mod-1: " + std::to_string(column[c]) + " appears twice";
                else seen |= 1u << column[c];
            }
        }
    }
    if (why) *why = w;
    return w.empty();
}

DemapperHip::DemapperHip(int framesize, int n_mod, const float* points_re_im, const uint8_t* column, int max_frames, int device)
    : DeviceStage(device), table_(true), max_frames_(max_frames)
{
    std::string why;
    if (!demap_table_check(n_mod, points_re_im, column, &why)) { err_.argument(why); return; }
    if (framesize != DVBS2_FECFRAME_NORMAL && framesize != DVBS2_FECFRAME_MEDIUM && framesize != DVBS2_FECFRAME_SHORT) { err_.argument("framesize must be DVBS2_FECFRAME_SHORT, _NORMAL or _MEDIUM"); return; }
    if (max_frames_ < 1 || max_frames_ > 65535) { err_.argument("max_frames must be in 1..65535 (frames are one launch dimension)"); return; }
    n_llr_ = framesize == DVBS2_FECFRAME_NORMAL ? 64800 : framesize == DVBS2_FECFRAME_MEDIUM ? 32400 : 16200;
    n_mod_ = n_mod;
    constellation_ = -1;
    points_.assign(points_re_im, points_re_im + (2 << n_mod));
    for (int c = 0; c < n_mod; c++) {
        column_[c] = column ? column[c] : (uint8_t)c;
        if (column_[c] != c) order_ = -1; // not the natural order
        cols_ |= (uint64_t)column_[c] << (8 * c);
        pos_ |= (uint64_t)c << (8 * column_[c]);
    }
    if (n_mod == 4 && order_ == 0) { // the same LLRs from the built-in 16APSK kernel, which measured 10 % faster at this size
        table_as_apsk_ = true;
        for (int i = 0; i < 16; i++) { apsk_.re[i] = points_[2 * i]; apsk_.im[i] = points_[2 * i + 1]; }
    }
    DeviceGuard guard(device);
    if (!guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the constellation table", alloc(&d_table_, points_.size()));
    HIP_OK(hipMemcpy(d_table_, points_.data(), points_.size() * sizeof(float), hipMemcpyHostToDevice));
}

void DemapperHip::table(int* n_mod, float* points_re_im, uint8_t* column) const
{
    if (n_mod) *n_mod = n_mod_;
    if (points_re_im) std::memcpy(points_re_im, points_.data(), points_.size() * sizeof(float));
    if (column) std::memcpy(column, column_, (size_t)n_mod_);
}

void DemapperHip::launch_table(const float* d_syms, int n_frames, const float* d_n0, int n0_count, int8_t* d_llr, hipStream_t stream)
{
    const int rows = n_syms(), quads = (rows + 3) / 4;
    const dim3 grid((quads + 255) / 256, n_frames);
    const float4* t = reinterpret_cast<const float4*>(d_table_);
#define DVBS2_TABLE_CASE(N) case N: hipLaunchKernelGGL(demap_table_kernel<N>, grid, dim3(256), 0, stream, d_syms, d_n0, n0_count, d_llr, rows, t, pos_); break
    switch (n_mod_) {
        DVBS2_TABLE_CASE(2); DVBS2_TABLE_CASE(3); DVBS2_TABLE_CASE(4); DVBS2_TABLE_CASE(5); DVBS2_TABLE_CASE(6); DVBS2_TABLE_CASE(8);
    }
#undef DVBS2_TABLE_CASE
}

void DemapperHip::launch_table_snr(const float* d_syms, const int8_t* d_ref_llr, int n_frames, float* d_snr, hipStream_t stream)
{
    hipLaunchKernelGGL(demap_snr_table_kernel, dim3(n_frames), dim3(256), 0, stream, reinterpret_cast<const float2*>(d_syms), d_ref_llr, d_snr,
                       n_syms(), n_mod_, reinterpret_cast<const float2*>(d_table_), cols_);
}

} // namespace dvbs2
