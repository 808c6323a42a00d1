// ldpc_node_plain.hpp -- the plain check node: one row of a regular layer, one edge at a time (every build's layer 0, the builds without
// packed nodes, and the parity-in-records kernel).
#pragma once
#include "ldpc_prims.hpp"

namespace dvbs2 {

// One check node (layered_decoder.hh:56-77 + algorithms.hh:170-192,203-206), fully unrolled for its degree.
// LLRs are offset-binary bytes Lb = L + 128 in LDS; messages are offset-binary bytes, 4 per dword.
// The kernel is VALU-issue bound (not HBM bound): ~22 VALU + 2 LDS instructions per edge.
//
// Parity links. Classic layout (PR = false): both parity LLRs live in LDS like the data LLRs. "Parity in records"
// (PR = true, low-rate tables, see ldpc_kernel_pr.hpp): parity row i is only ever touched by thread j of layers i and
// i+1, so it never needs LDS -- the own-parity LLR arrives in `own_in` (byte 7 of the NEXT layer's message
// record, where layer i+1 left it in the previous sweep), the previous-parity LLR is `carry` (what this thread's
// own-parity link produced one layer ago), the new own-parity LLR becomes the carry and the new previous-parity
// LLR is returned in byte 7 of this layer's record. Only row q-1 (own parity of the LAST layer, previous
// parity of layer 0 shifted by one lane) stays in LDS.
template <int DEG, bool LAYER0, bool PR = false, bool LAST = false, bool TC = false>
__device__ __forceinline__ void check_node(uint8_t* __restrict__ lds /*the whole LDS array*/, const uint32_t* ent /*uniform: S0, thr pairs*/,
                                           int jj, int lb /*byte offset of this frame's region*/, const uint32_t* mw, uint32_t* nm,
                                           int own_in = 0, int* carry = nullptr)
{
    constexpr bool OWN_REG = PR && !LAST;     // entry DEG-2
    constexpr bool PREV_REG = PR && !LAYER0;  // entry DEG-1
    // Issue priority RISES as the wave advances through the node (0 while it computes addresses and issues its LDS
    // reads, 1 for the reduction, 3 from the output phase until the next node starts): a wave that holds its data
    // is served before one that is about to wait for LDS anyway. Measured on B4: classic kernel 95.5 k -> 103.5 k
    // frames/s, parity-in-records 104.4 k -> 105.5 k; the opposite order costs 8 %.
    __builtin_amdgcn_s_setprio(0);
    int ad[DEG], Lb[DEG];
    const int jjb = jj + lb, jjb360 = jjb - kM;
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        // address = S0 + jj, minus 360 when jj >= thr; the two parity entries have rot = 0 (never wrap) except
        // the previous-parity entry of layer 0 (rot = 359)
        if (k >= DEG - 2 && !(LAYER0 && k == DEG - 1)) ad[k] = jjb + (int)ent[2 * k];
        else ad[k] = wrap_addr(jj, jjb, jjb360, ent[2 * k], ent[2 * k + 1]);
    }
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        if (OWN_REG && k == DEG - 2) Lb[k] = own_in;
        else if (PREV_REG && k == DEG - 1) Lb[k] = *carry;
        else Lb[k] = lds_rdx<TC>(ad[k]);
    }
    // check (0,0) has no previous-parity link (layered_decoder.hh:56,63-66)
    const bool last_valid = !LAYER0 || jj != 0;
    int spare = 0x80;

    int inp[DEG], mg[DEG];
    int min0 = 127, min1 = 127, signs = 0;
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        const int mb = (int)((mw[k >> 2] >> (8 * (k & 3))) & 0xffu);
        // R1 inp = sat8(L - m); R2 mag = usat(qabs(inp) - 1) == med3(|L - m| - 1, 0, 126)
        int d = min(max(Lb[k] - mb, -128), 127);
        int mag = mag_raw(Lb[k], mb);
        if (LAYER0 && k == DEG - 1) { d = last_valid ? d : 0; mag = last_valid ? mag : kMagAbsent; }
        inp[k] = d; mg[k] = mag;
        signs ^= d; // R4 xor of the sign bits
    }
    __builtin_amdgcn_s_setprio(1);
    two_smallest<DEG>(mg, min0, min1); // R3 on raw magnitudes; R2's clamp once per check
    min0 = clamp_mag(min0); min1 = clamp_mag(min1);
    const int s01 = min0 + min1;
    int msgc[4 * ((DEG + 3) / 4)];
#pragma unroll
    for (int k = 0; k < 4 * ((DEG + 3) / 4); k++) msgc[k] = 0;
#pragma unroll
    for (int k = 0; k < DEG; k++) {
        // R5 out = vsign(mag == min0 ? min1 : min0, (signs ^ x) | 127); mag is min0 or >= min1, so the selected
        // magnitude is min0 + min1 - min(mag, min1)
        const int other = s01 - vmed3_i32(mg[k], min0, min1);
        const int sg = (signs ^ inp[k]) >> 31;
        const int out = (other ^ sg) - sg;
        // R6 LLR = sat8(inp + out) with the unclamped out; R7 stored message = clamp(out, -32, 31)
        const int nl = sat_sum_u8(inp[k], out);
        if (OWN_REG && k == DEG - 2) *carry = nl;
        else if (PREV_REG && k == DEG - 1) spare = nl;
        else if (!(LAYER0 && k == DEG - 1) || last_valid) lds_wrx<TC>(ad[k], nl);
        msgc[k] = min(max(out, -32), 31);
    }
    __builtin_amdgcn_s_setprio(3);
    // two's-complement low bytes ^ 0x80 = offset binary
#pragma unroll
    for (int w = 0; w < (DEG + 3) / 4; w++)
        nm[w] = pack4_lo8(msgc[4 * w], msgc[4 * w + 1], msgc[4 * w + 2], msgc[4 * w + 3]) ^ 0x80808080u;
    if (PR) { // byte 7 of the record carries the previous-parity LLR (DEG <= 7)
        const uint32_t w1 = ((DEG + 3) / 4 > 1) ? nm[1] : 0x80808080u;
        nm[1] = (w1 & 0x00ffffffu) | ((uint32_t)spare << 24);
    }
}

} // namespace dvbs2
