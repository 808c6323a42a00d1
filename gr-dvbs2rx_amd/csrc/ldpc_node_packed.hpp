// ldpc_node_packed.hpp -- the packed check nodes: pairs of edges in the 16-bit halves of one register (check_node_v2, regular layers) and
// the single-pair hazard layer as a register chain walked in float (check_node_chain_v2), with the helpers they share with the packed
// phases of check_node_hazard (ldpc_node_hazard.hpp) and with check_node_v2_pr (ldpc_kernel_pr.hpp).
#pragma once
#include "ldpc_prims.hpp"

namespace dvbs2 {

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed check node ("v2", regular layers other than layer 0). The sweep is bound by VALU issue slots, so the node is
// built to need fewer of them per edge:
//   * ADDRESSES. Records are per WAVE (the host knows which 64 rows a wave owns): for an entry whose wrap point lies
//     outside the wave's rows the window offset is pre-adjusted (S0 or S0 - 360) and the address is ONE add; the few
//     entries whose wrap point falls inside the wave ("mixed", on average deg / 6) sit in the first NFIX slots and get
//     + 360 on the lanes below the wrap point under an EXEC mask taken from the record (one more add). 1.3 instead of 4
//     VALU instructions per edge.
//   * ARITHMETIC on PAIRS of edges in the halves of one register, as value << 8 in signed 16 bit: the saturating packed
//     add / subtract then IS the reference's int8 saturation (R1 sat8(L - m), R6 sat8(inp + out)), the message clamp (R7)
//     is one packed max + min per pair, |inp| is packed max(d, 0 - d). A positive saturation leaves 0xff in the low
//     byte of a half; nothing below lets it reach a result (see the notes at the uses).
//   * MAGNITUDES are reduced in packed form too (two_smallest_pk: a tree of sorted pairs per half position, one cross-half step
//     with swapped operand halves), the selection "mag == min0 ? min1 : min0" is T - clamp(mag, B0, B1) = T - min(mag, B1)
//     with B0 = min0, B1 = B0 + (min1' - min0'), T = min1' + B0, where x' = max(x - 1, 0) (R2's offset and floor applied once
//     per check, not per edge), and the sign goes onto T and the clamped magnitude before the subtraction (pair_out).
//     Census of the degree-7 node in the degree class 8 (tools/node_census.py): 108 -> 94 VALU instructions, 385 -> 345
//     issue cycles per wave (notes/r07_packed_node.md).
// Messages of such a layer are two's complement bytes (this layer's records are private to it: layer 0 and hazard
// layers keep offset binary); logical entry e = 2 j + h of pair j lives in dword j / 2, byte (j & 1) + 2 h, so that both
// pairs of a dword unpack with one instruction each. LLR bytes in LDS stay offset binary (shared with the other paths).
typedef short v2s16 __attribute__((ext_vector_type(2)));
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2s16 as_v2s(uint32_t x) { return __builtin_bit_cast(v2s16, x); }
__device__ __forceinline__ uint32_t as_u32(v2s16 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ void lds_wr_hi(int a, uint32_t v) { *reinterpret_cast<lds_byte_t*>((size_t)(uint32_t)a) = (uint8_t)(v >> 16); } // ds_write_b8_d16_hi

// Message storage of the packed nodes: one byte per message (R7 clamps a stored message to six bits, clamp(out, -32, 31)), pair j in
// bytes (j & 1) and (j & 1) + 2 of word j / 2. (Six-bit fields, five per dword, measured slower on table B4, 4096 frames: 107 k frames/s
// with byte messages, 93 k with six-bit fields at the same traffic, 85-91 k with the traffic actually reduced by a quarter -- the
// unpacking costs more than the bytes bring: the regular layers are limited by VALU issue and memory traffic at the same time.)
__device__ __forceinline__ uint32_t msg_pair16(const uint32_t* mw, int j)
{
    const uint32_t w = mw[j >> 1];
    return (j & 1) ? (w & 0xff00ff00u) : __builtin_amdgcn_perm(w, 0u, 0x060c040cu); // bytes 2, 0 of w to bytes 3, 1
}
template <int NP>
__device__ __forceinline__ void msg_pack16(const uint32_t* R /*clamped messages << 8 in both halves, pad half zero*/, uint32_t* nm)
{
#pragma unroll
    for (int w = 0; w < (NP + 1) / 2; w++)
        nm[w] = (2 * w + 1 < NP) ? ((R[2 * w] >> 8) | R[2 * w + 1]) : (R[2 * w] >> 8);
}
// msg_pack16 with the pad half of an odd degree still in R[NP - 1]: one v_perm per word instead of shift + or, and the pad byte is
// selected as zero instead of masked.
template <int NP, bool ODD>
__device__ __forceinline__ void msg_pack16_hb(uint32_t* R, uint32_t* nm)
{
#pragma unroll
    for (int w = 0; w < (NP + 1) / 2; w++) {
        const bool two = 2 * w + 1 < NP;                        // word w holds pairs 2w and 2w + 1
        const bool pad_lo = ODD && !two, pad_hi = ODD && two && 2 * w + 1 == NP - 1;
        const uint32_t sel = 0x01u | (two ? 0x05u : 0x0cu) << 8 | (pad_lo ? 0x0cu : 0x03u) << 16 | ((two && !pad_hi) ? 0x07u : 0x0cu) << 24;
        nm[w] = __builtin_amdgcn_perm(two ? R[2 * w + 1] : 0u, R[2 * w], sel); // bytes 1, 3 of pair 2w -> 0, 2; of pair 2w + 1 -> 1, 3
    }
}

// R3 on pairs: the two smallest of the 2 NP halves of a[] (all of them real: the caller lifts a pad above every magnitude). Per half
// position a tree of sorted pairs (min / max of two registers, then merges of two sorted pairs in four instructions), then ONE
// cross-half step with swapped operand halves (op_sel): m0 / m1 come out in BOTH halves. 3 NP - 4 + 4 packed instructions, against
// DEG extractions + the v_min3 / v_med3 network of two_smallest on scalars.
__device__ __forceinline__ v2s16 swap16(v2s16 x) { return __builtin_shufflevector(x, x, 1, 0); }
template <int NP>
__device__ __forceinline__ void two_smallest_pk(const v2s16* a, v2s16& m0, v2s16& m1)
{
    static_assert(NP >= 2, "two pairs at least");
    constexpr int NS = (NP + 1) / 2;
    v2s16 lo[NS], hi[NS]; // sorted pairs; a lone register has no second element (0x7fff: never below a magnitude)
#pragma unroll
    for (int k = 0; k < NS; k++) {
        if (2 * k + 1 < NP) { lo[k] = __builtin_elementwise_min(a[2 * k], a[2 * k + 1]); hi[k] = __builtin_elementwise_max(a[2 * k], a[2 * k + 1]); }
        else { lo[k] = a[2 * k]; hi[k] = (v2s16){ 0x7fff, 0x7fff }; }
    }
#pragma unroll
    for (int w = 1; w < NS; w *= 2) {
#pragma unroll
        for (int k = 0; k + w < NS; k += 2 * w) {
            const bool lone = (NP & 1) && k + w == NS - 1; // the lone register (never a receiver) has no second element: merge in three
            const v2s16 l = __builtin_elementwise_min(lo[k], lo[k + w]), x = __builtin_elementwise_max(lo[k], lo[k + w]);
            hi[k] = __builtin_elementwise_min(x, lone ? hi[k] : __builtin_elementwise_min(hi[k], hi[k + w]));
            lo[k] = l;
        }
    }
    const v2s16 s0 = swap16(lo[0]);
    m0 = __builtin_elementwise_min(lo[0], s0);
    m1 = __builtin_elementwise_min(__builtin_elementwise_max(lo[0], s0), __builtin_elementwise_min(hi[0], swap16(hi[0])));
}

// R5 - R7 of one pair (regular entries of the packed nodes). d: inp << 8, a: |inp| << 8 (>= B0 on every real half), B1p: B1 in both
// halves, Tt: T in both halves ^ tm, tm: all ones when the check's sign product is negative. The sign of an output is S = sg ^ tm with
// sg the sign mask of inp, and with S all ones or zero per half  (other ^ S) - S  ==  (T ^ S) - (c ^ S)  for other = T - c: the two
// xors are one v_bitop3 each and the negation costs no packed instruction of its own. clamp(a, B0, B1) is min(a, B1): a >= min0 >= B0.
// nl: the new LLR bytes of the pair in bits 0-7 and 16-23 (ds_write_b8 / ds_write_b8_d16_hi); R: the stored messages (R7) << 8.
// sum_out: where the caller wants the new LLRs of the pair as they go to LDS, still << 8 in the halves (the parity carry of the run loop).
// (Taking the sign mask once per pair in the caller's input phase, with |d| = sat((d ^ sg) - sg), was built for the run-loop form and
// measured 0.24 % SLOWER on B4 than this form: notes/r11_parity_carry.md.)
template <bool TC>
__device__ __forceinline__ void pair_out(v2s16 d, v2s16 a, v2s16 B1p, uint32_t Tt, uint32_t tm, uint32_t& nl, uint32_t& R, uint32_t* sum_out = nullptr)
{
    const v2s16 c = __builtin_elementwise_min(a, B1p);
    const uint32_t sg = as_u32(d >> (v2s16){ 15, 15 });
    uint32_t cs; // c ^ sg ^ tm as ONE v_bitop3 (the compiler splits a visible xor chain into two xors and re-associates Tt's)
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(cs) : "v"(as_u32(c)), "v"(sg), "v"(tm));
    const v2s16 out = as_v2s(Tt ^ sg) - as_v2s(cs);
    // R6: LLR = sat8(inp + out); the low byte of a half never reaches the byte that is stored. (The shift is opaque to the compiler:
    // it folds a visible one into the >> 16 of the second byte and stores that with a plain ds_write_b8 behind a second shift.)
    const uint32_t sum = as_u32(__builtin_elementwise_add_sat(d, out)) ^ kObPair<TC>;
    asm("v_lshrrev_b32 %0, 8, %1" : "=v"(nl) : "v"(sum));
    if (sum_out) *sum_out = sum;
    // R7
    R = as_u32(__builtin_elementwise_min(__builtin_elementwise_max(out, (v2s16){ -32 * 256, -32 * 256 }), (v2s16){ 31 * 256, 31 * 256 }));
}

// RUN: the form for trips of the run loop (kRun in ldpc_kernel.hpp), same values, fewer issue slots and no scalar bookkeeping in the address phase:
//   * the wrap fix is a SELECT of the base instead of an add under EXEC: jjb360 = jjb + 360 is loop invariant, a fix slot takes one
//     v_cndmask_b32 on the record's lane mask and then the one add of every other entry (per slot: 3 scalar instructions fewer, and
//     no asm statement that fences the scheduler);
//   * PARITY CARRY. A parity bit lies in two checks, c and c + 1: row j of layer i owns it (slot DEG - 2) and row j of layer i + 1 meets it
//     again as its previous parity (slot DEG - 1), so the same THREAD writes the byte in one trip and reads it back in the next, and
//     nobody else touches it in between. Inside a run it stays in a register: `carry` holds the new LLRs of the pair with the own-parity
//     entry as pair_out adds them up (LDS form, << 8 in the halves; the entry is byte 3 of it for an odd degree, byte 1 for an even one).
//     The node takes its previous-parity input out of it -- with the v_perm that assembles the pair anyway, which also drops the low
//     byte a saturated input leaves in a half --, neither reads that byte from LDS nor writes its own parity byte, and leaves the new
//     carry. The run loop loads the carry in front of a run's first trip and writes the last own-parity byte behind its last one
//     (ldpc_kernel.hpp); the planner vouches, for every record a run can take, that own parity lies 360 bytes behind previous parity, that
//     neither is a fix slot, and that the two slots of consecutive records of a run name the same byte (ldpc_plan.cpp, parity_chain_ok).
template <int DEG, int DMAX, bool TC, bool RUN = false, class Prefetch>
__device__ __forceinline__ void check_node_v2(const uint32_t* ent /*record words 4..: S0w[DMAX], then (mask lo, mask hi)[NFIX]*/,
                                              int jjb, const uint32_t* mw, uint32_t* nm, Prefetch prefetch_next_record, int jjb360 = 0 /*RUN: jjb + 360*/,
                                              uint32_t* carry = nullptr /*RUN*/)
{
    constexpr int NP = (DEG + 1) / 2;      // pairs
    constexpr int NFIX = v2_nfix(DMAX) < DEG - 2 ? v2_nfix(DMAX) : DEG - 2; // parity entries never wrap
    constexpr bool ODD = (DEG & 1) != 0;   // the upper half of the last pair is a pad: L = m = 0, magnitude "absent"
    __builtin_amdgcn_s_setprio(0);
    int ad[DEG];
    auto addresses = [&]() {
        if constexpr (RUN) {
#pragma unroll
            for (int k = 0; k < DEG; k++)
                if (k != DEG - 2) ad[k] = (k < NFIX ? wrap_base(jjb, jjb360, ent[DMAX + 2 * k], ent[DMAX + 2 * k + 1]) : jjb) + (int)ent[k];
            ad[DEG - 2] = 0; // the own-parity byte is read 360 bytes behind the previous-parity one (parity_chain_ok) and not written: no address of its own
            return;
        }
#pragma unroll
        for (int k = 0; k < DEG; k++) ad[k] = jjb + (int)ent[k];
#pragma unroll
        for (int k = 0; k < NFIX; k++) ad[k] = fix_wrap(ad[k], ent[DMAX + 2 * k], ent[DMAX + 2 * k + 1]);
    };
    addresses();
    int Lb[DEG];
#pragma unroll
    for (int k = 0; k < DEG - (RUN ? 2 : 0); k++) Lb[k] = lds_rd(ad[k]);
    if constexpr (RUN) { Lb[DEG - 2] = lds_rd_at<kM>(ad[DEG - 1]); Lb[DEG - 1] = 0; } // (the previous-parity byte comes out of the carry)
    v2s16 d[NP], a[NP];
    uint32_t sx = 0;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const uint32_t M = msg_pair16(mw, j); // messages of pair j: << 8 in both halves
        const uint32_t hi = (ODD && j == NP - 1) ? (TC ? 0x00u : 0x80u) : (uint32_t)Lb[2 * j + 1];
        // (RUN, last pair: previous parity is its low half for an odd degree -- byte 3 of the carry -- and its high half for an even one -- byte 1)
        const uint32_t Lp = !(RUN && j == NP - 1) ? __builtin_amdgcn_perm(hi, (uint32_t)Lb[2 * j], 0x040c000cu)
                            : ODD ? __builtin_amdgcn_perm(hi, *carry, 0x040c030cu) : __builtin_amdgcn_perm(*carry, (uint32_t)Lb[2 * j], 0x050c000cu);
        const uint32_t L = Lp ^ kObPair<TC>; // -> two's complement << 8
        d[j] = __builtin_elementwise_sub_sat(as_v2s(L), as_v2s(M));           // R1 (a half that saturates upwards reads 0x7fff)
        sx ^= as_u32(d[j]);                                                   // R4: bits 15 and 31 collect the signs
        a[j] = __builtin_elementwise_max(d[j], __builtin_elementwise_sub_sat(as_v2s(0u), d[j])); // |inp| << 8 (0x7fff for -128 and for saturated halves)
    }
    __builtin_amdgcn_s_setprio(1);
    // (Issuing the NEXT layer's scalar record loads from this point -- scalar memory shares its counter with LDS, so a load in
    // flight turns every LDS wait into "wait for everything" -- was tried with a scheduling barrier and an ordering dependency:
    // it cost 9 % on table B4 and a factor 4 on the degree-30 class through what it does to register allocation. The loads stay
    // at the top of the layer; notes/history.md 3.4.)
    // RUN: the run loop's trip issues the NEXT record's scalar loads from here, into the ping-pong record set that is dead during the node
    // (the layer loop has one set and paid sixteen s_mov for the attempt above). The input phase's LDS wait no longer covers scalar loads and
    // is counted over the byte reads; the header is first needed at the trip's end (notes/r12_trip_waits.md).
    if constexpr (RUN) prefetch_next_record(); else (void)prefetch_next_record;
    if (ODD) a[NP - 1] = as_v2s(as_u32(a[NP - 1]) | 0x7fff0000u); // the pad's magnitude: above every real one
    v2s16 m0, m1;
    two_smallest_pk<NP>(a, m0, m1);
    // the low byte (0xff after a saturation) is dropped HERE, once per check: every selected magnitude below is B1-clamped,
    // so a 0x7fff among the inputs can only come out as the clean 0x7f00 level it stands for
    const int n0 = (int)(as_u32(m0) & 0x7f00u), n1 = (int)(as_u32(m1) & 0x7f00u);
    // R2: mag = max(|inp| - 1, 0), applied to the two minima (monotone); unsigned saturating subtract (full rate)
    const int n0m = (int)__builtin_elementwise_sub_sat((uint32_t)n0, 256u), n1m = (int)__builtin_elementwise_sub_sat((uint32_t)n1, 256u);
    const int B1 = n0 + n1m - n0m, T = n1m + n0;
    const uint32_t tm = (uint32_t)((int)(sx ^ (sx << 16)) >> 31); // all ones when the number of negative inputs is odd
    const v2s16 B1p = { (short)B1, (short)B1 };
    const uint32_t Tt = __builtin_amdgcn_perm((uint32_t)T, (uint32_t)T, 0x01000100u) ^ tm; // T in both halves (one v_perm; the compiler's own broadcast is a multiply)
    uint32_t R[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) {
        uint32_t nl;
        pair_out<TC>(d[j], a[j], B1p, Tt, tm, nl, R[j], RUN && j == (DEG - 2) / 2 ? carry : nullptr);
        if (!(RUN && 2 * j == DEG - 2)) lds_wr(ad[2 * j], (int)nl); // (RUN: the own-parity byte, slot DEG - 2, stays in the carry)
        if (!(ODD && j == NP - 1) && !(RUN && 2 * j + 1 == DEG - 2)) lds_wr_hi(ad[2 * j + 1], nl);
    }
    __builtin_amdgcn_s_setprio(3);
    msg_pack16_hb<NP, ODD>(R, nm);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Hazard layer with ONE pair (two entries X, Y of one group, block B <= kChainMaxBlock), packed arithmetic, register chain.
// The host orders the pair so that X's bit of row r is Y's bit of row r + B: row r hands its new X value to row r + B.
//   heads  r < B            X and Y both original                       -> Y written at once, X starts the chain
//   middle B <= r < 360-B   X original, Y = X of row r - B (chain)
//   tails  r >= 360 - B     X = Y of head r + B - 360 (in LDS after the heads), Y from the chain; final writer of X
// Phases (frame barriers between them): P1 all rows: regular entries read and reduced (packed, as check_node_v2); heads also
// resolve their pair. P2 rows >= B: read X, publish the chain operands of their row as four floats. P3 the B head lanes walk
// r -> r + B: six VALU instructions per step on exact small integers in float (fma, two med3 with a negated operand, sub,
// add, clamp) plus one 16-byte read and one 4-byte log write; a lone wave issues one instruction per ~4 cycles, so the step
// costs its instruction count. P4 all rows: pair completed from the log, final minima, outputs of every entry, messages.
// Identical to the reference's row order: a bit of the pair is touched by exactly two rows, the later one sees the earlier one.
//   chain step for row r with incoming Y value c (offset binary 0..255):  x = sigma (c - 128 - mY),
//   out = sgn(x) min(P, max(|x| - 1, 0)) = w - sgn(w), w = clamp(x, -(P+1), P+1);  c' = clamp(inpX + 128 + out, 0, 255)
__device__ __forceinline__ float as_f32(uint32_t x) { return __builtin_bit_cast(float, x); }
__device__ __forceinline__ float vmed3_f32(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
__device__ __forceinline__ float byte1_f32(uint32_t x) { return (float)((x >> 8) & 0xffu); } // v_cvt_f32_ubyte1

template <int DEG, int DMAX, bool TC>
__device__ __forceinline__ void check_node_chain_v2(const uint32_t* ent /*S0w[DMAX], masks[NFIX + 2]*/, int jj, int jjb, bool work, int B,
                                                    const uint32_t* mw, uint32_t* nm, lds_u32_t* tab /*LDS scratch, 16-byte aligned*/,
                                                    volatile lds_i32_t* hb_ctr, int& hb_epoch, const int hb_lane)
{
    constexpr int NP = (DEG + 1) / 2;
    constexpr int NFIXH = (v2_nfix(DMAX) + 2) < DEG - 2 ? (v2_nfix(DMAX) + 2) : DEG - 2;
    constexpr bool ODD = (DEG & 1) != 0;
    constexpr bool KEEP_AD = DEG <= 16; // high degrees recompute the addresses in P4 instead of holding 30 registers across the phases
    lds_v4f_t* rec = reinterpret_cast<lds_v4f_t*>(tab);           // [360 + B] chain operands
    lds_f32_t* logv = reinterpret_cast<lds_f32_t*>(tab) + 4 * (kM + kChainMaxBlock); // [360 + B] value that arrived at row r
    const bool head = work && jj < B, body = work && jj >= B;
    const bool middle = body && jj + B < kM; // rows whose new X value travels down the chain; the others (tails) end a chain
    int LbX = 0x80;
    int ad[DEG];
    v2s16 d[NP], a[NP];
    uint32_t sxp = 0;
    int p0 = 0x7fff, p1 = 0x7fff;
    int Pm = 0;
    float c = 0.f;
    __builtin_amdgcn_s_setprio(0);
    auto addresses = [&]() {
#pragma unroll
        for (int k = 0; k < DEG; k++) ad[k] = jjb + (int)ent[k];
#pragma unroll
        for (int k = 0; k < NFIXH; k++) ad[k] = fix_wrap(ad[k], ent[DMAX + 2 * k], ent[DMAX + 2 * k + 1]);
    };
    auto pair0 = [&](int LbX, int LbY) { // d, |d| of the pair [X | Y] (LLR bytes as they lie in LDS)
        const uint32_t L = __builtin_amdgcn_perm((uint32_t)LbY, (uint32_t)LbX, 0x040c000cu) ^ kObPair<TC>;
        const uint32_t M = msg_pair16(mw, 0);
        d[0] = __builtin_elementwise_sub_sat(as_v2s(L), as_v2s(M));
        a[0] = __builtin_elementwise_max(d[0], __builtin_elementwise_sub_sat(as_v2s(0u), d[0]));
    };
    if (work) {
        addresses();
        int Lb[DEG];
#pragma unroll
        for (int k = 2; k < DEG; k++) Lb[k] = lds_rd(ad[k]);
        int LbY = 0x80;
        if (head) { LbX = lds_rd(ad[0]); LbY = lds_rd(ad[1]); }
        else if (middle) LbX = lds_rd(ad[0]); // original value: the only other row that touches this bit comes later (row jj + B)
#pragma unroll
        for (int j = 1; j < NP; j++) {
            const uint32_t M = msg_pair16(mw, j);
            const uint32_t hi = (ODD && j == NP - 1) ? (TC ? 0x00u : 0x80u) : (uint32_t)Lb[2 * j + 1];
            const uint32_t L = __builtin_amdgcn_perm(hi, (uint32_t)Lb[2 * j], 0x040c000cu) ^ kObPair<TC>;
            d[j] = __builtin_elementwise_sub_sat(as_v2s(L), as_v2s(M));
            sxp ^= as_u32(d[j]);
            a[j] = __builtin_elementwise_max(d[j], __builtin_elementwise_sub_sat(as_v2s(0u), d[j]));
        }
        int mg[DEG - 2];
#pragma unroll
        for (int k = 2; k < DEG; k++) mg[k - 2] = (k & 1) ? (int)(as_u32(a[k >> 1]) >> 16) : (int)(as_u32(a[k >> 1]) & 0xffffu);
        two_smallest<DEG - 2>(mg, p0, p1); // raw |inp| << 8 of the regular entries (a pad never enters: DEG - 2 real values)
        Pm = (int)(__builtin_elementwise_sub_sat((uint32_t)(p0 & 0x7f00), 256u) >> 8); // R2 on the partial minimum: 0..126
        if (head) {
            pair0(LbX, LbY);
            // the other entry of the pair is the only input outside the partial: |out_X| = min(Pm, mag Y) and vice versa
            const uint32_t sw = __builtin_amdgcn_alignbit(as_u32(a[0]), as_u32(a[0]), 16) & 0x7f007f00u;
            const v2u16 mgs = __builtin_elementwise_sub_sat(__builtin_bit_cast(v2u16, sw), (v2u16){ 256, 256 });
            const v2s16 other = __builtin_elementwise_min(__builtin_bit_cast(v2s16, mgs), (v2s16){ (short)(Pm << 8), (short)(Pm << 8) });
            const uint32_t par = (uint32_t)((int)(sxp ^ (sxp << 16)) >> 31);
            const uint32_t ds = __builtin_amdgcn_alignbit(as_u32(d[0]), as_u32(d[0]), 16);
            const v2s16 sg = as_v2s(ds ^ par) >> (v2s16){ 15, 15 };
            const v2s16 out = as_v2s(as_u32(other) ^ as_u32(sg)) - sg;
            const uint32_t raw = as_u32(__builtin_elementwise_add_sat(d[0], out));
            const uint32_t nl = raw ^ 0x80008000u;                      // offset binary in bytes 1 and 3 (the chain walks offset-binary values)
            lds_wr_hi(ad[1], (TC ? raw : nl) >> 8);                    // Y now (a tail row reads it as its X)
            c = byte1_f32(nl);                   // X starts the chain
        }
    }
    // chain operands of the middle rows (a tail row only receives: the walker logs what arrives there and needs nothing from it)
    if (middle) {
        const uint32_t L = __builtin_amdgcn_perm(TC ? 0x00u : 0x80u, (uint32_t)LbX, 0x040c000cu) ^ kObPair<TC>;
        const uint32_t M0 = msg_pair16(mw, 0);
        const uint32_t M = M0 & 0x0000ffffu;
        const v2s16 dx = __builtin_elementwise_sub_sat(as_v2s(L), as_v2s(M));       // [inp_X | 0]
        const uint32_t fold = sxp ^ (sxp << 16);                                      // bit 31: parity of the signs of the regular entries (the inputs other than X and Y)
        const float sigma = as_f32(0x3f800000u | (fold & 0x80000000u));
        const int mY = (int)M0 >> 24;                                                 // Y's message (upper half of the pair, << 8)
        v4f32 r;
        r.x = sigma;
        r.y = -sigma * (float)(128 + mY);
        r.z = (float)(Pm + 1);
        r.w = byte1_f32(as_u32(dx) ^ 0x8000u);                  // inp_X + 128
        rec[jj] = r;
    }
    lds_barrier();
    if (head) {
        // rows past 359 read the padding of the table and log into the padding: no per-lane predicate in the loop
        const lds_v4f_t* rp = rec + jj + B;
        lds_f32_t* lp = logv + jj + B;
        const int nsteps = (kM - 1) / B; // rows jj + k B, k = 1 .. nsteps (the last one may lie in the padding)
        __builtin_amdgcn_s_setprio(3);
        auto step = [&](const v4f32 rc) {
            *lp = c; lp += B;
            const float x = __builtin_fmaf(c, rc.x, rc.y);
            const float w = vmed3_f32(x, -rc.z, rc.z);
            const float f = w - vmed3_f32(w, -1.f, 1.f);
            c = vmed3_f32(rc.w + f, 0.f, 255.f);
        };
        // A step is six dependent instructions (~40 cycles of a lone wave), an LDS read takes 64-130: with the operands of only the
        // NEXT row in flight the walk ran at the LDS latency (~150 cycles per step, cycle stamps of round 3: 26.6 k cycles for the 179
        // steps of 3/4 normal's block-2 layer). Four rows are kept in flight; reads past the table (rows >= 360 + block) fetch
        // whatever lies there and are never used.
        v4f32 q0 = rp[0], q1 = rp[B], q2 = rp[2 * B], q3 = rp[3 * B];
        rp += 4 * B;
        int k = 0;
        for (; k + 4 <= nsteps; k += 4) {
            step(q0); q0 = rp[0];
            step(q1); q1 = rp[B];
            step(q2); q2 = rp[2 * B];
            step(q3); q3 = rp[3 * B];
            rp += 4 * B;
        }
        if (k < nsteps) { step(q0); k++; }
        if (k < nsteps) { step(q1); k++; }
        if (k < nsteps) { step(q2); k++; }
        __builtin_amdgcn_s_setprio(0);
    }
    lds_barrier();
    if (work) {
        if constexpr (!KEEP_AD) addresses();
        if (body) {
            if (!middle) LbX = lds_rd(ad[0]); // tail: the Y value its head wrote in the first phase
            pair0(LbX, (int)logv[jj] ^ (TC ? 0x80 : 0)); // (the log holds the chain's offset-binary values)
        }
        sxp ^= as_u32(d[0]);
        int m4[4] = { p0, p1, (int)(as_u32(a[0]) & 0xffffu), (int)(as_u32(a[0]) >> 16) };
        int n0, n1;
        two_smallest<4>(m4, n0, n1);
        n0 &= 0x7f00; n1 &= 0x7f00;
        const int n0m = (int)__builtin_elementwise_sub_sat((uint32_t)n0, 256u), n1m = (int)__builtin_elementwise_sub_sat((uint32_t)n1, 256u);
        // outputs in the pair form of check_node_v2 (pair_out: min(a, B1) for the clamp -- every real half, the pair's included, is >= n0 --,
        // the sign applied before the subtraction, one shift for both LLR bytes) and its one-v_perm message packing
        const int B1 = n0 + n1m - n0m, T = n1m + n0;
        const v2s16 B1p = { (short)B1, (short)B1 };
        const uint32_t tm = (uint32_t)((int)(sxp ^ (sxp << 16)) >> 31);
        const uint32_t Tt = __builtin_amdgcn_perm((uint32_t)T, (uint32_t)T, 0x01000100u) ^ tm;
        uint32_t R[NP];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NP; j++) {
            uint32_t nl;
            pair_out<TC>(d[j], a[j], B1p, Tt, tm, nl, R[j]);
            if (j == 0) {
                if (jj + B >= kM) lds_wr(ad[0], (int)nl);   // a tail row is the last writer of its X bit (the others handed X down the chain)
                if (body) lds_wr_hi(ad[1], nl);             // heads wrote Y in P1 (by now a tail row may have replaced it)
            } else {
                lds_wr(ad[2 * j], (int)nl);
                if (!(ODD && j == NP - 1)) lds_wr_hi(ad[2 * j + 1], nl);
            }
        }
        __builtin_amdgcn_s_setprio(3);
        msg_pack16_hb<NP, ODD>(R, nm);
    }
}

} // namespace dvbs2
