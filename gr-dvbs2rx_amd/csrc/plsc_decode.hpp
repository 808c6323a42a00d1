// plsc_decode.hpp -- the one-wavefront PLSC decoder shared by the PLFRAME front end (plframe_hip.hip, one wavefront per
// frame) and the frame tracker (plsync_hip.hip, one wavefront per stream): closed-loop de-rotation by the SOF phase
// (reference lib/pl_freq_sync.cc:429-436), pi/2 BPSK decisions (lib/pi2_bpsk.cc:45-196) and the RM(64,7) decoder
// (lib/reed_muller.cc:120-210); and the small device steps more than one PL kernel unit takes: wave_sum, the two ways of removing
// the pi/2 BPSK modulation, wrap_pi. The PLHEADER constants and bit rule are pl_signal.h's. The functions of namespace plsc are device
// code; those that exchange across lanes expect all 64 lanes of the wavefront active.
// NOT here: the four-way Rn de-scrambling switch of pl_payload_kernel and pl_estimate_kernel. As a function, in either form (returned
// pair, out-parameters, forced inline), it changes the order of the merge block's predecessors and with it the packed arithmetic the
// compiler forms behind it in pl_payload_kernel (notes/pl_signal.md); the two statements stay until a change that may move kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pl_signal.h" // kSofWord, kPlscScrambler, plheader_bit

namespace dvbs2 {
namespace plsc {

constexpr float kS = 0.7071067811865476f;
constexpr double kPi = 3.14159265358979323846;

__device__ inline float wave_sum(float v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m); // a + b is commutative: every lane ends with the same bits
    return v;
}

// Two ways of taking the pi/2 BPSK modulation off PLHEADER symbol k, kept side by side ON PURPOSE: they round differently.
// remove_modulation: x_k * conj(h_k), conj(h_k) = rot[k & 1] * (1 - 2 bit), rot = { (S, -S), (-S, -S) } (lib/pi2_bpsk.cc:23-34, :57-60):
// four products by S and two sums, the reference's values (plframe, plsync).
__device__ inline float2 remove_modulation(float2 x, int k, int bit)
{
    const float sg = bit ? -1.0f : 1.0f;
    const float cr = ((k & 1) ? -kS : kS) * sg, ci = -kS * sg;
    return make_float2(x.x * cr - x.y * ci, x.x * ci + x.y * cr);
}
// unmod: x_k conj(h_k) sqrt(2), conj(h_k) sqrt(2) = ((k odd ? -1 : 1), -1) (1 - 2 bit) (lib/pi2_bpsk.cc:18-43), so each component is one
// sum or difference of the two input components: one rounding, no multiply (plcoarse, where the common scale does not reach an angle).
__device__ inline float2 unmod(float2 x, int k, int bit)
{
    const float sg = bit ? -1.0f : 1.0f;
    const float cr = (k & 1) ? -sg : sg, ci = -sg;
    return make_float2(x.x * cr - x.y * ci, x.x * ci + x.y * cr);
}

// a phase difference back into [-pi, pi] (lib/pl_freq_sync.cc:166-171, :280-285): compared and corrected in double, kept as float
__device__ inline float wrap_pi(float d)
{
    if ((double)d > kPi) d = (float)((double)d - 2.0 * kPi);
    else if ((double)d < -kPi) d = (float)((double)d + 2.0 * kPi);
    return d;
}

// the data-aided sum over the SOF (lib/pl_freq_sync.cc:217-220); lane l < 26 passes PLHEADER symbol l
__device__ inline float2 sof_sum(float2 x_l, int l)
{
    const float2 t0 = remove_modulation(x_l, l, l < 26 ? plheader_bit(0, l) : 0);
    const bool in_sof = l < 26;
    return make_float2(wave_sum(in_sof ? t0.x : 0.0f), wave_sum(in_sof ? t0.y : 0.0f));
}

// The PLSC of one PLHEADER (lib/plsync_cc_impl.cc:582-590). Lane l passes xa = PLHEADER symbol 26 + l (PLSC symbol l) and
// xb = PLHEADER symbol 25 + l; rank[c] is the position of codeword c in the enabled list, 255 = disabled. Every lane
// returns the decoded value.
__device__ inline int decode_wave(float2 xa, float2 xb, float sof_phase, int l, const uint8_t* __restrict__ rank, int coherent, int soft)
{
    float sn, cs;
    sincosf(-sof_phase, &sn, &cs);
    const float2 ya = make_float2(xa.x * cs - xa.y * sn, xa.x * sn + xa.y * cs);
    const int scr = (int)((kPlscScrambler >> (63 - l)) & 1);
    float v; // the descrambled soft decision, or +-1 for a descrambled hard decision
    if (coherent) {
        const float rr = (l & 1) ? -kS : kS, ri = -kS;
        const float sd = ya.x * rr - ya.y * ri; // real(x rot[j & 1]) (lib/pi2_bpsk.cc:45-74, :181-196)
        if (soft) v = scr ? -sd : sd;
        else v = ((sd < 0.0f) != (scr != 0)) ? -1.0f : 1.0f;
    } else {
        // differential: bit_j = bit_{j-1} ^ (imag(conj(y_{j+1}) y_j) < 0) ^ (j & 1), starting from the last SOF bit 0
        // (lib/pi2_bpsk.cc:165-176): a prefix parity over the lanes
        const float2 yb = make_float2(xb.x * cs - xb.y * sn, xb.x * sn + xb.y * cs);
        const float dim = ya.x * yb.y - ya.y * yb.x;
        const unsigned long long flips = __ballot(((dim < 0.0f) ? 1 : 0) ^ (l & 1));
        const unsigned long long upto = l == 63 ? ~0ull : ((2ull << l) - 1ull);
        const int bit = __popcll(flips & upto) & 1;
        v = (bit != scr) ? -1.0f : 1.0f;
    }
    // RM(64,7) as a transform (lib/reed_muller.cc:72-96): the first stage forms the pair sums (even lanes, b7 = 0) and
    // pair differences (odd lanes, b7 = 1); five more stages are a 32-point Walsh-Hadamard transform over lane bits
    // 1..5. Lane 2 w + b7 then holds the metric of codeword (bitrev5(w) << 2) | b7, and its negative that of the
    // codeword with bit 1 (the all-ones row) set. On +-1 inputs every value is a small integer: exact in float.
    for (int m = 1; m < 64; m <<= 1) {
        const float o = __shfl_xor(v, m);
        v = (l & m) ? o - v : v + o;
    }
    const int c0 = (int)((__brev((unsigned)(l >> 1)) >> 27) << 2) | (l & 1), c1 = c0 | 2;
    const int r0 = rank[c0], r1 = rank[c1];
    if (coherent && soft) {
        // maximum inner product over ALL 128 entries, those of disabled codewords being 0.0; first maximum wins
        // (lib/reed_muller.cc:203-209)
        const float m0 = r0 != 255 ? v : 0.0f, m1 = r1 != 255 ? -v : 0.0f;
        float bv = m1 > m0 ? m1 : m0; int bi = m1 > m0 ? c1 : c0;
        for (int m = 1; m < 64; m <<= 1) {
            const float ov = __shfl_xor(bv, m); const int oi = __shfl_xor(bi, m);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        return bi;
    }
    // minimum Hamming distance, FIRST minimum in the order of the enabled list (lib/reed_muller.cc:128-141):
    // distance = (64 -+ W) / 2; key = distance | position in the list | codeword
    const int w = (int)v;
    const unsigned k0 = r0 != 255 ? (unsigned)(((64 - w) >> 1) << 16 | r0 << 8 | c0) : 0xffffffffu;
    const unsigned k1 = r1 != 255 ? (unsigned)(((64 + w) >> 1) << 16 | r1 << 8 | c1) : 0xffffffffu;
    unsigned key = k0 < k1 ? k0 : k1;
    for (int m = 1; m < 64; m <<= 1) { const unsigned o = __shfl_xor(key, m); key = o < key ? o : key; }
    return (int)(key & 127u);
}

} // namespace plsc
} // namespace dvbs2
