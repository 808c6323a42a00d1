// ldpc_node_hazard.hpp -- the hazard check node (check_node_hazard): a layer in which two or more entries of one group make the
// reference's strictly ordered update visible. First phase, one of the ordered-phase strategies, last phase.
#pragma once
#include "ldpc_prims.hpp"
#include "ldpc_node_packed.hpp"

namespace dvbs2 {

template <int DMAX, bool HZ2> constexpr bool kTlc = tlc_class(DMAX) && !HZ2; // two-level lane chain (check_node_hazard): the classes of tlc_class (ldpc_layout.h)
constexpr int kTlcLowRegMinDmax = 24; // from this degree class on a two-level-chain layer keeps its regular entries in the low-register form

// constants of check_node_hazard's ordered phase
constexpr int kFwalkMaxDeg = 12;     // largest check degree of a single-pair lane chain walked in float (kFloatWalk)
constexpr int kTlcFwalkMinDmax = 24; // the near pair of a two-level lane chain walked in float (six instructions per row, 16-byte operand records)
                                     // in the packed hazard nodes from this degree class up -- measured (round 5): 5/6 normal +3.1 %, 9/10 normal
                                     // +0.35 %; 3/4 normal (class 16) -2.0 %
// The switches of check_node_hazard, by name. A call site says which ones it sets (HazardCfg); the rest keep these defaults.
struct HazardSwitches {
    bool layer0 = false;        // layer 0: check (0,0) has no previous-parity link (see check_node)
    bool pr = false, last = false; // parity in records, and its last layer (see check_node)
    bool two_level = false;     // two-level walk compiled in
    bool low_reg = false;       // low-register form: a regular entry keeps ONE word pm = |Lb - mb| << 8 | (inp & 0xff) between the phases and its address is computed twice (two-level-chain layers of the classes >= 24)
    bool tlc = false;           // two-level walk with the near pair as a LANE CHAIN (round 3), see below
    bool chain_ok = true;       // false: no lane chain in this build (the 80-VGPR build since round 4, see kLaneChainBuilt)
    bool class8 = false;        // the kernel of the degree class <= 8: early pair reads, walk on absolute addresses (kEarlyPair)
    bool packed_phases = false; // round 5: FIRST and LAST phase in the packed form of check_node_v2 (pairs of regular entries in the halves of one
                                // register, one-add addresses from this wave's record, two's complement messages in pair-byte order); the ordered
                                // phase in between is untouched. `ent` is then the per-wave record: S0w[dmaxv], lane masks of the first NFIXH slots
    int dmaxv = 0;              // the degree class whose per-wave record format `ent` has (packed_phases)
    bool tc = false;            // LLR bytes in LDS are two's complement (the builds with packed nodes)
};
// The configuration type check_node_hazard takes: a call builds it from the switches it sets, each by its name:
//   check_node_hazard<DEG, NC, HazardCfg<hz::layer0<true>, hz::tc<TC>>>(...)
// (Types at namespace scope on purpose: with a class local to the kernel as the argument the node's instantiations get internal linkage, and
// that alone moved the register allocation of the one-frame builds.)
#define DVBS2_HZ_SWITCH(NAME, TYPE) template <TYPE V> struct NAME { static constexpr void set(HazardSwitches& s) { s.NAME = V; } };
namespace hz {
DVBS2_HZ_SWITCH(layer0, bool) DVBS2_HZ_SWITCH(pr, bool) DVBS2_HZ_SWITCH(last, bool) DVBS2_HZ_SWITCH(two_level, bool) DVBS2_HZ_SWITCH(low_reg, bool)
DVBS2_HZ_SWITCH(tlc, bool) DVBS2_HZ_SWITCH(chain_ok, bool) DVBS2_HZ_SWITCH(class8, bool) DVBS2_HZ_SWITCH(packed_phases, bool) DVBS2_HZ_SWITCH(dmaxv, int)
DVBS2_HZ_SWITCH(tc, bool)
}
#undef DVBS2_HZ_SWITCH
template <class... Set> constexpr HazardSwitches hazard_switches() { HazardSwitches s{}; (Set::set(s), ...); return s; }
template <class... Set> struct HazardCfg { static constexpr HazardSwitches sw = hazard_switches<Set...>(); };

// Hazard layer (two or more entries of one group, ldpc_schedule.h): the reference's strictly ordered update
// makes check j see what checks j' < j wrote to the bits they share. Only the NC hazard entries (placed first)
// carry that dependency, so the check node is split in three:
//   P1  all 360 rows in parallel: regular entries are read and reduced to a partial (min0, min1, signs);
//   P2  ascending blocks of B_i rows, one workgroup barrier per block: the rows of the block read their
//       hazard bits (now final with respect to all earlier rows), complete (min0, min1, signs), and write the
//       hazard bits back;
//   P3  all rows in parallel: outputs of the regular entries.
// The result is identical to the sequential order: inside a block no two rows share a bit, blocks ascend, and
// a regular entry's bits are touched by exactly one row of the layer.
// NC (2, 4 or 8) is the number of entries handled in P2: the hazard entries, rounded up with regular data entries
// (moving a regular entry into the ordered part does not change the result).
template <int DEG, int NC, class Cfg>
__device__ __forceinline__ void check_node_hazard(uint8_t* __restrict__ lds, const uint32_t* ent, int jj, int lb, bool work,
                                                  int block, int block2 /*two-level walk: rows per outer block, 0 = off*/, const uint32_t* mw, uint32_t* nm, int own_in, int* carry,
                                                  lds_u32_t* tab /*lane_chain_words(block) of LDS scratch when the layer is a lane chain*/,
                                                  volatile lds_i32_t* hb_ctr, int& hb_epoch, const int hb_lane /*frame barrier state*/,
                                                  unsigned long long* ph = nullptr /*timing builds: cycles per phase of this node (8 slots), else null*/)
{
    constexpr bool LAYER0 = Cfg::sw.layer0, PR = Cfg::sw.pr, LAST = Cfg::sw.last, TWO = Cfg::sw.two_level, LR = Cfg::sw.low_reg, TLC = Cfg::sw.tlc,
                   CHAINOK = Cfg::sw.chain_ok, CLASS8 = Cfg::sw.class8, V2P = Cfg::sw.packed_phases, TC = Cfg::sw.tc;
    constexpr int DMAXV = Cfg::sw.dmaxv;
    unsigned long long tph = ph ? __builtin_readcyclecounter() : 0ull;
#define DVBS2_PH(i) do { if (ph) { const unsigned long long t_ = __builtin_readcyclecounter(); ph[i] += t_ - tph; tph = t_; } } while (0)
    constexpr bool OWN_REG = PR && !LAST;     // entry DEG-2 (see check_node)
    constexpr bool PREV_REG = PR && !LAYER0;  // entry DEG-1
    static_assert(!(LR && PR), "the low-register form is for the classic layout");
    static_assert(!V2P || (!LAYER0 && !PR && !LR && (NC % 2) == 0 && DEG - NC >= 2), "packed phases: regular layers of the classic layout, ordered entries in pairs");
    // ---- packed first / last phase (V2P): state of the regular PAIRS between the phases (check_node_v2) ----
    constexpr int NP = (DEG + 1) / 2;                  // pairs; pairs 0 .. NC/2 - 1 hold the ordered entries
    constexpr int NPH = NC / 2;
    constexpr bool ODD = (DEG & 1) != 0;               // the upper half of the last pair is a pad
    constexpr int NFIXH = V2P ? ((DMAXV / 2) < DEG - 2 ? (DMAXV / 2) : DEG - 2) : 0; // fix slots of the record: the NC ordered entries first, then the mixed regular ones
    constexpr bool KEEP_AD = !V2P || DEG <= 16;        // high degrees compute the regular entries' addresses again in the last phase
    v2s16 dP[V2P ? NP : 1], aP[V2P ? NP : 1];
    uint32_t sxp = 0;
    constexpr int NAD = LR ? NC : DEG; // LR: only the ordered entries keep their addresses
    int ad[NAD], inp[LR ? NC : DEG], mg[LR ? NC : DEG];
    int pm[LR ? DEG : 1];  // LR: regular entry k keeps pm[k]
    // Lane-chain layers of the low degree classes: the pair's two LLR bytes are read WITH the regular entries (one LDS round trip for all
    // seven instead of three in a row on the wave that walks the chain afterwards). A value read here is used only by the rows for which
    // no earlier row of this layer writes that bit: entry 0 of the rows below 360 - block, entry 1 of the heads.
    // Measured (round 4, interleaved A/B, whole tables): degree <= 8: B4 +0.7 %, 9/20 ... S2_TABLE_B3 +1.8 %, B1 +1 %, B2 -0.6 %; degree class
    // 12: 3/5 normal 0, 2/3 normal and T2 2/3 -4 % (register allocation of their one-frame builds) -- and the degree-5..8 instantiations
    // INSIDE the class-12 kernel cost its tables 3-7 % as well (S2X 99/180 ... S2X_TABLE_B4 -7 %), so the switch is the kernel's class
    // (CLASS8 = DMAX <= 8), not the check degree.
    constexpr bool kEarlyPair = CLASS8 && NC == 2 && !LR && !PR && CHAINOK && !V2P;
    int Lh01[2] = { 0x80, 0x80 };
    int p0 = 0, p1 = 0;
    const int jjb = jj + lb, jjb360 = jjb - kM;
    int min0 = 127, min1 = 127, signs = 0;
    int spare = 0x80;
    const bool last_valid = !LAYER0 || jj != 0;
    auto addr = [&](int k) -> int {
        if (k >= DEG - 2 && !(LAYER0 && k == DEG - 1)) return jjb + (int)ent[2 * k];
        return wrap_addr(jj, jjb, jjb360, ent[2 * k], ent[2 * k + 1]);
    };
    __builtin_amdgcn_s_setprio(0); // as in check_node; the ordered steps below run at the top priority
    auto v2p_addresses = [&](int first) { // one add per entry from this wave's record (+ 360 under the record's lane mask in the fix slots)
#pragma unroll
        for (int k = 0; k < DEG; k++) if (k >= first) ad[k] = jjb + (int)ent[k];
#pragma unroll
        for (int k = 0; k < NFIXH; k++) if (k >= first) ad[k] = fix_wrap(ad[k], ent[DMAXV + 2 * k], ent[DMAXV + 2 * k + 1]);
    };
    if constexpr (V2P) {
        if (work) {
            v2p_addresses(0);
            int Lb[DEG];
#pragma unroll
            for (int k = NC; k < DEG; k++) Lb[k] = lds_rd(ad[k]);
#pragma unroll
            for (int j = NPH; j < NP; j++) {
                const uint32_t M = msg_pair16(mw, j);
                const uint32_t hi = (ODD && j == NP - 1) ? (TC ? 0x00u : 0x80u) : (uint32_t)Lb[2 * j + 1];
                const uint32_t L = __builtin_amdgcn_perm(hi, (uint32_t)Lb[2 * j], 0x040c000cu) ^ kObPair<TC>;
                dP[j] = __builtin_elementwise_sub_sat(as_v2s(L), as_v2s(M));
                sxp ^= as_u32(dP[j]);
                aP[j] = __builtin_elementwise_max(dP[j], __builtin_elementwise_sub_sat(as_v2s(0u), dP[j]));
            }
            int mgr[DEG - NC];
#pragma unroll
            for (int k = NC; k < DEG; k++) mgr[k - NC] = (k & 1) ? (int)(as_u32(aP[k >> 1]) >> 16) : (int)(as_u32(aP[k >> 1]) & 0xffffu);
            two_smallest<DEG - NC>(mgr, p0, p1); // raw |inp| << 8 of the regular entries
            min0 = (int)(__builtin_elementwise_sub_sat((uint32_t)(p0 & 0x7f00), 256u) >> 8); // R2 on the partial minimum: 0 .. 126 (what the ordered phase takes)
            signs = (int)(sxp ^ (sxp << 16));                                                  // bit 31: parity of the regular entries' signs (the only bit the ordered phase looks at)
        }
    } else
    if constexpr (LR) {
        if (work) {
#pragma unroll
            for (int k = 0; k < NC; k++) ad[k] = addr(k);
#pragma unroll
            for (int k = NC; k < DEG; k++) {
                const int Lb = lds_rdx<TC>(addr(k));
                const int mb = (int)((mw[k >> 2] >> (8 * (k & 3))) & 0xffu);
                int d = min(max(Lb - mb, -128), 127);
                const int magp = (int)__builtin_amdgcn_sad_u16((uint32_t)Lb, (uint32_t)mb, 0u);
                if (LAYER0 && k == DEG - 1) { d = last_valid ? d : 0; pm[k] = last_valid ? pm_pack(magp, d) : (kMagAbsent << 8); }
                else pm[k] = pm_pack(magp, d);
                signs ^= d;
            }
            two_smallest<DEG - NC>(pm + NC, p0, p1);
            min0 = pm_min_clamped(p0); min1 = pm_min_clamped(p1);
        }
    } else
    if (work) {
#pragma unroll
        for (int k = 0; k < DEG; k++) {
            if (k >= DEG - 2 && !(LAYER0 && k == DEG - 1)) ad[k] = jjb + (int)ent[2 * k];
            else ad[k] = wrap_addr(jj, jjb, jjb360, ent[2 * k], ent[2 * k + 1]);
        }
#pragma unroll
        for (int k = 0; k < DEG; k++) {
            if (kEarlyPair && k < 2) Lh01[k] = lds_rdx<TC>(ad[k]); // (see the lane chain below: issued with the regular reads, used only where still valid)
            if (k >= NC) { // regular entry
                const int Lb = (OWN_REG && k == DEG - 2) ? own_in : (PREV_REG && k == DEG - 1) ? *carry : lds_rdx<TC>(ad[k]);
                const int mb = (int)((mw[k >> 2] >> (8 * (k & 3))) & 0xffu);
                int d = min(max(Lb - mb, -128), 127);
                int mag = mag_raw(Lb, mb);
                if (LAYER0 && k == DEG - 1) { d = last_valid ? d : 0; mag = last_valid ? mag : kMagAbsent; }
                inp[k] = d; mg[k] = mag;
                signs ^= d;
            }
        }
        two_smallest<DEG - NC>(mg + NC, min0, min1); // raw magnitudes of the regular entries (see mag_raw)
        min0 = clamp_mag(min0); min1 = clamp_mag(min1);
    }
    DVBS2_PH(0); // P1: regular entries read and reduced
    if constexpr (!V2P) {
#pragma unroll
    for (int w = 0; w < (DEG + 3) / 4; w++) nm[w] = 0;
    }
    // P2 keeps only what the NEXT block needs on its critical path: the new hazard LLRs. For hazard entry k the
    // magnitude sent back is the minimum over all OTHER entries = min(partial min0 of the regular entries, the
    // other hazard magnitudes) and the sign is the xor of all other signs; the merge of the hazard entries into
    // (min0, min1, signs) for P3 and the hazard message bytes are computed after the loop.
    if (PR && (DEG + 3) / 4 < 2) nm[1] = 0;
    int hout[NC], hmb[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) {
        hout[k] = 0; inp[k] = 0; mg[k] = 127;
        if constexpr (V2P) hmb[k] = (int)(((mw[k >> 2] >> (8 * (((k >> 1) & 1) + 2 * (k & 1)))) & 0xffu) ^ 0x80u); // pair-byte order, two's complement -> offset binary
        else hmb[k] = (int)((mw[k >> 2] >> (8 * (k & 3))) & 0xffu);
    }
    // One ordered step per block of `block` rows. A step is a chain of dependent instructions of a single wave (the
    // next block reads what this one wrote), so its length is what a hazard layer costs: rel = jj - start is kept
    // incrementally (one subtract + one unsigned compare select the rows of the block).
    __builtin_amdgcn_s_setprio(3);
    bool lane_chain = false;
    // (the low-register form has room for it at every degree)
    constexpr bool kLaneChainBuilt = NC == 2 && (LR || V2P || DEG <= kLaneChainMaxDeg) && !PR && CHAINOK;
    if constexpr (kLaneChainBuilt) lane_chain = tab != nullptr; // wave-uniform (header bit 12)
    if constexpr (kLaneChainBuilt) if (lane_chain) {
        // LANE CHAIN (one hazard pair, block <= 128, host-ordered so that entry 0's bit of row r is entry 1's bit of
        // row r + block). A lone wave issues one instruction per 4-7 cycles whatever it is, so an ordered step costs
        // its instruction count: the recurrence r -> r + block is walked by the `block` lanes that own rows
        // 0..block-1 with the chained LLR in a register, ~20 instructions per step, no exec-mask bookkeeping, no LDS
        // hand-over, no barrier per step; everything else happens before and after, in parallel over all rows. Round 3: two
        // barriers per layer instead of four (cycle stamps, DVBS2_PH: the heads' step, the publishing pass and their barriers
        // cost a chain layer of table B4 ~1.4 k of its ~5 k cycles):
        //   A  together with the first phase (no barrier in between): rows < 360 - block read entry 0 -- no earlier row of
        //      this layer writes that bit -- ; the heads (rows < block, nothing precedes them) do their full two-entry step and
        //      write entry 1 at once (the only reader of that bit is the tail row r + 360 - block, after the walk); the other
        //      rows publish {inp0, partial min0, partial sign, message byte 1}                             | barrier
        //   C  chain lanes: incoming entry-1 LLR -> new entry-0 LLR of row r, incoming value logged      | barrier
        //   D  rows >= block: (tails first read entry 0 = what their head wrote in A) complete both outputs from the
        //      logged value; write entry 1; the last row of a chain also writes entry 0 (in the reference's order it is the
        //      final writer of that bit). No barrier towards the outputs of the regular entries: other bits.
        // (The walk on exact small integers in float -- six instructions per step as in the packed chain node instead of ~20 -- was
        // measured here too in round 3: the 16-byte operand records and the float state cost every build of every degree class 4-6
        // VGPRs; B4 113.2 k -> 112.4 k, the 80-VGPR and one-frame builds -4 ... -8 %. It stays in the packed chain node.)
        lds_byte_t* ulog = reinterpret_cast<lds_byte_t*>(tab + kM + block); // after the per-row records (360 rows + one block of padding)
        int chained = 0x80;
        // Round 4, degree class 8: the walk on exact small integers in float with the operands of FOUR rows in flight. The
        // integer step is ~17 dependent VALU instructions and one record read ahead: a lone wave needs ~110 cycles per row either way
        // (issue ~4 cycles per instruction, an LDS read 100-130), 1.4 k cycles for the 8-10 rows of table B4's chains. In float the step is
        // six instructions (fma, two med3 with a negated operand, sub, add, clamp -- the packed chain node's step, check_node_chain_v2)
        // and with four 16-byte records in flight the LDS latency is covered.
        //   record of row r: { sigma, -sigma m1, P + 1, inp0 + 128 }  (sigma = +-1: partial sign; m1: entry 1's message, offset binary;
        //   P: partial minimum); incoming entry-1 LLR c (offset binary):  x = sigma (c - m1), w = clamp(x, -(P+1), P+1),
        //   out = w - sgn(w) = sgn(x) min(P, max(|x| - 1, 0)),  c' = clamp(inp0 + 128 + out, 0, 255)
        // Largest check degree that walks in float -- measured (round 4, interleaved A/B): 8 -> B2 +8 %, B4 +0.5 %; 12 -> 3/5 normal +1 %,
        // T2 2/3 +4 %, the one-frame class-12 tables +5 %; 16 -> B7 -1 %; 28 -> 8/9 normal -8 %, 5/6 -3 %.
        constexpr bool kFloatWalk = DEG <= kFwalkMaxDeg && !LR && !PR;
        lds_v4f_t* frec = lds_align16<lds_v4f_t>(tab);                                                   // [360 + block]
        lds_f32_t* flog = reinterpret_cast<lds_f32_t*>(frec) + 4 * (kM + kChainMaxBlock);              // [360 + block]
        auto publish = [&]() {
            if constexpr (kFloatWalk) {
                const float sigma = as_f32(0x3f800000u | ((uint32_t)signs & 0x80000000u));
                v4f32 r;
                r.x = sigma; r.y = -sigma * (float)hmb[1]; r.z = (float)(min0 + 1); r.w = (float)(inp[0] + 128);
                frec[jj] = r;
            } else
            tab[jj] = ((uint32_t)inp[0] & 0x1ffu) | ((uint32_t)min0 << 9) | (((uint32_t)signs >> 31) << 16) | ((uint32_t)hmb[1] << 24);
        };
        const bool head = work && jj < block, body = work && jj >= block;
        // (degrees above 20 without the low-register form keep the round-2 order -- heads | barrier | publishing | barrier | walk |
        // barrier | completion | barrier --: reading entry 0 inside the first phase costs the degree class 28 sixteen more spilled
        // registers and table B10 7 %)
        constexpr bool kTwoBarrier = LR || DEG <= 20;
        const bool orig0 = work && (kTwoBarrier ? jj + block < kM : jj < block); // entry 0 still holds its value from before the layer (every head is one: block <= 128)
        if (orig0) {
            const int L0 = kEarlyPair ? Lh01[0] : lds_rdx<TC>(ad[0]);
            inp[0] = min(max(L0 - hmb[0], -128), 127);
            mg[0] = mag_raw(L0, hmb[0]);
        }
        if (head) {
            const int L1 = kEarlyPair ? Lh01[1] : lds_rdx<TC>(ad[1]);
            inp[1] = min(max(L1 - hmb[1], -128), 127);
            mg[1] = mag_raw(L1, hmb[1]);
            int o0, o1;
            asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(mg[1]), "v"(min0));
            asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o1) : "v"(mg[0]), "v"(min0));
            const int s0 = (signs ^ inp[1]) >> 31, s1 = (signs ^ inp[0]) >> 31;
            hout[0] = (o0 ^ s0) - s0;
            hout[1] = (o1 ^ s1) - s1;
            chained = sat_sum_u8(inp[0], hout[0]);
            lds_wrx<TC>(ad[1], sat_sum_u8(inp[1], hout[1]));
        } else if (kTwoBarrier && orig0)
            publish();
        if constexpr (!kTwoBarrier) {
            lds_barrier();
            if (body) { // every row below the heads, tails included (their entry 0 is what a head just wrote)
                const int L0 = lds_rdx<TC>(ad[0]);
                inp[0] = min(max(L0 - hmb[0], -128), 127);
                mg[0] = mag_raw(L0, hmb[0]);
                publish();
            }
        }
        DVBS2_PH(1); // chain heads + publishing
        lds_barrier();
        DVBS2_PH(3); // barrier
        if constexpr (kFloatWalk && CLASS8) { if (head) {
            // absolute LDS addresses, ONE running address for the records and one for the log (through typed pointers the compiler kept
            // eight offsets and added the array base at every access: four address instructions per step of a lone wave)
            int ra = (int)(uint32_t)(size_t)(frec + jj + block), la = (int)(uint32_t)(size_t)(flog + jj + block);
            const int rs = block * 16, ls = block * 4;
            auto ld = [](int a) -> v4f32 { return *reinterpret_cast<const lds_v4f_t*>((size_t)(uint32_t)a); };
            const int nsteps = (kM - 1) / block;
            float c = (float)chained;
            auto step = [&](const v4f32 rc) {
                *reinterpret_cast<lds_f32_t*>((size_t)(uint32_t)la) = c; la += ls;
                const float x = __builtin_fmaf(c, rc.x, rc.y);
                const float w = vmed3_f32(x, -rc.z, rc.z);
                const float f = w - vmed3_f32(w, -1.f, 1.f);
                c = vmed3_f32(rc.w + f, 0.f, 255.f);
            };
            v4f32 q0 = ld(ra), q1 = ld(ra + rs), q2 = ld(ra + 2 * rs), q3 = ld(ra + 3 * rs);
            ra += 4 * rs;
            int k = 0;
            for (; k + 4 <= nsteps; k += 4) {
                step(q0); q0 = ld(ra); ra += rs;
                step(q1); q1 = ld(ra); ra += rs;
                step(q2); q2 = ld(ra); ra += rs;
                step(q3); q3 = ld(ra); ra += rs;
            }
            if (k < nsteps) { step(q0); k++; }
            if (k < nsteps) { step(q1); k++; }
            if (k < nsteps) { step(q2); k++; }
        } } else
        if constexpr (kFloatWalk) { if (head) {
            const lds_v4f_t* rp = frec + jj + block;
            lds_f32_t* lp = flog + jj + block;
            const int nsteps = (kM - 1) / block; // rows jj + k block, k = 1 .. nsteps (the last one may lie in the padding)
            float c = (float)chained;
            auto step = [&](const v4f32 rc) {
                *lp = c; lp += block;
                const float x = __builtin_fmaf(c, rc.x, rc.y);
                const float w = vmed3_f32(x, -rc.z, rc.z);
                const float f = w - vmed3_f32(w, -1.f, 1.f);
                c = vmed3_f32(rc.w + f, 0.f, 255.f);
            };
            v4f32 q0 = rp[0], q1 = rp[block], q2 = rp[2 * block], q3 = rp[3 * block]; // (reads past the table fetch scratch that is never used)
            rp += 4 * block;
            int k = 0;
            for (; k + 4 <= nsteps; k += 4) {
                step(q0); q0 = rp[0];
                step(q1); q1 = rp[block];
                step(q2); q2 = rp[2 * block];
                step(q3); q3 = rp[3 * block];
                rp += 4 * block;
            }
            if (k < nsteps) { step(q0); k++; }
            if (k < nsteps) { step(q1); k++; }
            if (k < nsteps) { step(q2); k++; }
        } } else
        if (head) {
            // rows past 359 read the padding of the table and log into the padding: no per-lane predicate in the loop; the record
            // of a tail row (last of its chain) is not written: what is computed from it is never used
            const lds_u32_t* tp = tab + jj + block;
            lds_byte_t* up = ulog + jj + block;
            uint32_t t = *tp;
            for (int first = block; first < kM; first += block) {
                const uint32_t tc = t;
                tp += block;
                t = *tp; // next row's record, in flight during this step
                const int i0 = (int)(tc << 23) >> 23, P = (int)((tc >> 9) & 0x7fu), m1 = (int)(tc >> 24);
                const int sw = (int)(tc << 15); // partial sign in bit 31
                *up = (uint8_t)chained; up += block;
                const int i1 = min(max(chained - m1, -128), 127);
                const int g1 = mag_raw(chained, m1);
                int o0;
                asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(g1), "v"(P));
                const int s0 = (sw ^ i1) >> 31;
                chained = sat_sum_u8(i0, (o0 ^ s0) - s0);
            }
        }
        DVBS2_PH(4); // walk
        lds_barrier();
        DVBS2_PH(5); // barrier after the walk
        if (body) {
            if (kTwoBarrier && !orig0) { // tail: entry 0 = the entry-1 value its head wrote before the walk
                const int L0 = lds_rdx<TC>(ad[0]);
                inp[0] = min(max(L0 - hmb[0], -128), 127);
                mg[0] = mag_raw(L0, hmb[0]);
            }
            const int L1 = kFloatWalk ? (int)flog[jj] : (int)ulog[jj];
            inp[1] = min(max(L1 - hmb[1], -128), 127);
            mg[1] = mag_raw(L1, hmb[1]);
            int o0, o1;
            asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(mg[1]), "v"(min0));
            asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o1) : "v"(mg[0]), "v"(min0));
            const int s0 = (signs ^ inp[1]) >> 31, s1 = (signs ^ inp[0]) >> 31;
            hout[0] = (o0 ^ s0) - s0;
            hout[1] = (o1 ^ s1) - s1;
            lds_wrx<TC>(ad[1], sat_sum_u8(inp[1], hout[1]));
            if (jj + block >= kM) lds_wrx<TC>(ad[0], sat_sum_u8(inp[0], hout[0]));
        }
    }
    // TWO-LEVEL LANE CHAIN (NC >= 4, block2 > 0, header bit 12; degree class 32 without the heavy-hazard paths). As in the two-level
    // walk below, ONE pair of ordered entries (0, 1; host-ordered: entry 0's bit of row r is entry 1's bit of row r + block) is closer
    // than every other pair (>= block2 >= 2 block rows apart), and the rows are processed in outer blocks of block2 rows. Inside an
    // outer block only the near pair is sequential -- and it is walked like a single-pair lane chain: the `block` lanes that own rows
    // 0 .. block-1 carry the chained LLR in a register from row to row ACROSS the outer blocks, ~20 instructions per row, no LDS
    // hand-over. Per outer block:
    //   a  its rows read their far entries (final: the rows that share those bits lie in other outer blocks), fold them into the
    //      partial minimum / sign, read entry 0 (untouched so far, or -- last `block` rows -- what a head wrote in the first outer
    //      block) and publish {inp0, partial min, partial sign, message byte 1}; heads (first outer block) do their two-entry step | barrier
    //   b  the chain lanes walk the rows of this outer block, logging what arrives at each row                               | barrier
    //   c  its rows complete the near pair from the logged value, then the far entries (minimum over all other entries), and
    //      write those LLRs                                                                                                  | barrier
    // 9/10 normal, layer 5 (pairs 4, 53, 84, 86 rows apart): 90 eight-entry steps through LDS (~80 k cycles, a fifth of the sweep)
    // become 7 outer blocks + 89 register steps.
    constexpr bool kTlcBuilt = TLC && (NC == 4 || NC == 8) && !PR;
    bool tlc = false;
    if constexpr (kTlcBuilt) tlc = block2 > 0 && tab != nullptr; // wave-uniform
    if constexpr (kTlcBuilt) if (tlc) {
        lds_byte_t* ulog = reinterpret_cast<lds_byte_t*>(tab + kM + block);
        constexpr bool kTlcFloat = V2P && DMAXV >= kTlcFwalkMinDmax;
        lds_v4f_t* trec = lds_align16<lds_v4f_t>(tab);                                      // kTlcFloat: [360 + block] operand records { sigma, -sigma m1, P + 1, inp0 + 128 }
        lds_f32_t* tlog = reinterpret_cast<lds_f32_t*>(trec) + 4 * (kM + kChainMaxBlock); //            [360 + block] the value that arrived at a row
        int chained = 0x80;
        float cf = 0.f;
        const bool head = work && jj < block;
        int rnext = jj + block; // chain lanes: the next row to visit
        for (int sb = 0; sb < kM; sb += block2) {
            const int sb_end = min(sb + block2, kM);
            const bool in_sb = work && (uint32_t)(jj - sb) < (uint32_t)block2;
            int minF = min0, signsF = signs;
            if (in_sb) {
                int Lh[NC];
#pragma unroll
                for (int k = 2; k < NC; k++) Lh[k] = lds_rdx<TC>(ad[k]);
                const int L0 = lds_rdx<TC>(ad[0]);
#pragma unroll
                for (int k = 2; k < NC; k++) {
                    inp[k] = min(max(Lh[k] - hmb[k], -128), 127);
                    mg[k] = mag_offset(Lh[k], hmb[k]);
                    signsF ^= inp[k];
                    minF = min(minF, mg[k]);
                }
                inp[0] = min(max(L0 - hmb[0], -128), 127);
                mg[0] = mag_raw(L0, hmb[0]);
                if (head) { // (first outer block: block2 >= 2 block)
                    const int L1 = lds_rdx<TC>(ad[1]);
                    inp[1] = min(max(L1 - hmb[1], -128), 127);
                    mg[1] = mag_raw(L1, hmb[1]);
                    int o0, o1;
                    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(mg[1]), "v"(minF));
                    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o1) : "v"(mg[0]), "v"(minF));
                    const int s0 = (signsF ^ inp[1]) >> 31, s1 = (signsF ^ inp[0]) >> 31;
                    hout[0] = (o0 ^ s0) - s0;
                    hout[1] = (o1 ^ s1) - s1;
                    chained = sat_sum_u8(inp[0], hout[0]);
                    cf = (float)chained;
                    lds_wrx<TC>(ad[1], sat_sum_u8(inp[1], hout[1]));
                } else if constexpr (kTlcFloat) {
                    const float sigma = as_f32(0x3f800000u | ((uint32_t)signsF & 0x80000000u));
                    v4f32 r;
                    r.x = sigma; r.y = -sigma * (float)hmb[1]; r.z = (float)(minF + 1); r.w = (float)(inp[0] + 128);
                    trec[jj] = r;
                } else
                    tab[jj] = ((uint32_t)inp[0] & 0x1ffu) | ((uint32_t)minF << 9) | (((uint32_t)signsF >> 31) << 16) | ((uint32_t)hmb[1] << 24);
            }
            lds_barrier();
            if constexpr (kTlcFloat) { if (head && rnext < sb_end) {
                // (as the single-pair chains: x = sigma (c - m1), w = clamp(x, -(P+1), P+1), out = w - sgn(w), c' = clamp(inp0 + 128 + out, 0, 255))
                v4f32 q = trec[rnext];
                for (; rnext < sb_end; rnext += block) {
                    const v4f32 rc = q;
                    q = trec[rnext + block]; // next row's record (valid when that row belongs to this outer block; reloaded otherwise)
                    tlog[rnext] = cf;
                    const float x = __builtin_fmaf(cf, rc.x, rc.y);
                    const float w = vmed3_f32(x, -rc.z, rc.z);
                    const float f = w - vmed3_f32(w, -1.f, 1.f);
                    cf = vmed3_f32(rc.w + f, 0.f, 255.f);
                }
            } } else
            if (head && rnext < sb_end) {
                uint32_t t = tab[rnext];
                for (; rnext < sb_end; rnext += block) {
                    const uint32_t tc = t;
                    t = tab[rnext + block]; // next row's record (valid when that row belongs to this outer block; reloaded otherwise)
                    const int i0 = (int)(tc << 23) >> 23, P = (int)((tc >> 9) & 0x7fu), m1 = (int)(tc >> 24);
                    const int sw = (int)(tc << 15);
                    ulog[rnext] = (uint8_t)chained;
                    const int i1 = min(max(chained - m1, -128), 127);
                    const int g1 = mag_raw(chained, m1);
                    int o0;
                    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(g1), "v"(P));
                    const int s0 = (sw ^ i1) >> 31;
                    chained = sat_sum_u8(i0, (o0 ^ s0) - s0);
                }
            }
            lds_barrier();
            if (in_sb) {
                if (!head) {
                    const int L1 = kTlcFloat ? (int)tlog[jj] : (int)ulog[jj];
                    inp[1] = min(max(L1 - hmb[1], -128), 127);
                    mg[1] = mag_raw(L1, hmb[1]);
                    int o0, o1;
                    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(mg[1]), "v"(minF));
                    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o1) : "v"(mg[0]), "v"(minF));
                    const int s0 = (signsF ^ inp[1]) >> 31, s1 = (signsF ^ inp[0]) >> 31;
                    hout[0] = (o0 ^ s0) - s0;
                    hout[1] = (o1 ^ s1) - s1;
                    lds_wrx<TC>(ad[1], sat_sum_u8(inp[1], hout[1]));
                    if (jj + block >= kM) lds_wrx<TC>(ad[0], sat_sum_u8(inp[0], hout[0])); // last row of its chain: final writer of that bit
                }
                mg[0] = clamp_mag(mg[0]); mg[1] = clamp_mag(mg[1]); // (raw above; everything below and after the loop takes clamped ones)
                const int xall = signsF ^ inp[0] ^ inp[1];
                int pre[NC + 1], suf[NC + 1];
                pre[0] = min0; suf[NC] = 127;
#pragma unroll
                for (int k = 0; k < NC; k++) pre[k + 1] = min(pre[k], mg[k]);
#pragma unroll
                for (int k = NC - 1; k >= 0; k--) suf[k] = min(suf[k + 1], mg[k]);
#pragma unroll
                for (int k = 2; k < NC; k++) {
                    const int other = min(pre[k], suf[k + 1]);
                    const int sg = (xall ^ inp[k]) >> 31;
                    const int out = (other ^ sg) - sg;
                    hout[k] = out;
                    lds_wrx<TC>(ad[k], sat_sum_u8(inp[k], out));
                }
            }
            if (sb + block2 < kM) lds_barrier(); // the next outer block reads what this one wrote
        }
    }
    // TWO-LEVEL WALK (NC >= 4, block2 > 0). The block size B is the distance of the NEAREST hazard pair only; every other pair
    // of hazard entries is at least block2 >= 2 B rows apart. So the rows are walked in outer blocks of block2 rows: at its start the
    // rows of an outer block read their FAR hazard entries (2 .. NC-1: final with respect to all earlier outer blocks, untouched
    // inside this one) and fold them into the partial result; then only the near pair (entries 0, 1; host-ordered) goes through the
    // ordered steps of B rows -- a two-entry step instead of an NC-entry one -- and at the end of the outer block its rows write the
    // far entries back. 360 / B short steps + 360 / block2 long ones instead of 360 / B long ones (B11 layer 5: B = 4).
    bool two_level = false;
    // (degree 29 and above: only the eight-entry form is compiled -- every instantiation costs that class registers, and 9/10 normal,
    // the table it is there for, has its block-4 layer with eight ordered entries)
    constexpr bool kTwoBuilt = TWO && NC >= 4 && (DEG < 29 || NC == 8);
    if constexpr (kTwoBuilt) two_level = block2 > 0;
    if constexpr (kTwoBuilt) if (two_level) {
        for (int sb = 0; sb < kM; sb += block2) {
            const bool in_sb = work && (uint32_t)(jj - sb) < (uint32_t)block2;
            int minF = min0, signsF = signs;
            if (in_sb) {
                int Lh[NC];
#pragma unroll
                for (int k = 2; k < NC; k++) Lh[k] = lds_rdx<TC>(ad[k]);
#pragma unroll
                for (int k = 2; k < NC; k++) {
                    inp[k] = min(max(Lh[k] - hmb[k], -128), 127);
                    mg[k] = mag_offset(Lh[k], hmb[k]);
                    signsF ^= inp[k];
                    minF = min(minF, mg[k]);
                }
            }
            const int sb_end = min(sb + block2, kM);
            int rel = in_sb ? jj - sb : 0x40000000;
            for (int start = sb; start < sb_end; start += block, rel -= block) {
                if ((uint32_t)rel < (uint32_t)block) {
                    const int L0 = lds_rdx<TC>(ad[0]), L1 = lds_rdx<TC>(ad[1]);
                    inp[0] = min(max(L0 - hmb[0], -128), 127);
                    inp[1] = min(max(L1 - hmb[1], -128), 127);
                    mg[0] = mag_offset(L0, hmb[0]);
                    mg[1] = mag_offset(L1, hmb[1]);
                    const int o0 = min(mg[1], minF), o1 = min(mg[0], minF);
                    const int s0 = (signsF ^ inp[1]) >> 31, s1 = (signsF ^ inp[0]) >> 31;
                    hout[0] = (o0 ^ s0) - s0;
                    hout[1] = (o1 ^ s1) - s1;
                    lds_wrx<TC>(ad[0], sat_sum_u8(inp[0], hout[0]));
                    lds_wrx<TC>(ad[1], sat_sum_u8(inp[1], hout[1]));
                }
                if (start + block < sb_end && (start >> 6) != ((start + 2 * block - 1) >> 6)) lds_barrier();
            }
            if (in_sb) {
                const int xall = signsF ^ inp[0] ^ inp[1];
                int pre[NC + 1], suf[NC + 1];
                pre[0] = min0; suf[NC] = 127;
#pragma unroll
                for (int k = 0; k < NC; k++) pre[k + 1] = min(pre[k], mg[k]);
#pragma unroll
                for (int k = NC - 1; k >= 0; k--) suf[k] = min(suf[k + 1], mg[k]);
#pragma unroll
                for (int k = 2; k < NC; k++) {
                    const int other = min(pre[k], suf[k + 1]);
                    const int sg = (xall ^ inp[k]) >> 31;
                    const int out = (other ^ sg) - sg;
                    hout[k] = out;
                    lds_wrx<TC>(ad[k], sat_sum_u8(inp[k], out));
                }
            }
            // the next outer block reads what this one wrote: a barrier, unless both sit inside one and the same wavefront
            if ((sb >> 6) != ((sb + 2 * block2 - 1) >> 6)) lds_barrier();
        }
    }
    // (Round 4 measured the alternative to a workgroup barrier per block -- each wave takes only the steps of the blocks that hold its
    // rows, waits for a progress counter in LDS and goes on to its regular outputs while later waves still step: bit-exact and 4-11 %
    // SLOWER (9/10 normal -4 %, 3/5 -8 %, 8/9 -9 %, 2/3 -11 %): a hand-over through an LDS word costs ~300 cycles against ~30-50 for
    // s_barrier, more than the overlapped outputs give back. notes/r04_experiments.md.)
    int rel = (work && !lane_chain && !two_level && !tlc) ? jj : 0x40000000;
    for (int start = (lane_chain || two_level || tlc) ? kM : 0; start < kM; start += block, rel -= block) {
        if ((uint32_t)rel < (uint32_t)block) {
            if constexpr (NC == 2) {
                // two hazard entries: each one's magnitude sent back is min(partial min0, the other's magnitude) =
                // med3(raw other, 0, min0) (min0 is already clamped to [0, 126])
                const int L0 = lds_rdx<TC>(ad[0]), L1 = lds_rdx<TC>(ad[1]);
                inp[0] = min(max(L0 - hmb[0], -128), 127);
                inp[1] = min(max(L1 - hmb[1], -128), 127);
                mg[0] = mag_raw(L0, hmb[0]);
                mg[1] = mag_raw(L1, hmb[1]);
                int o0, o1;
                asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o0) : "v"(mg[1]), "v"(min0));
                asm("v_med3_i32 %0, %1, 0, %2" : "=v"(o1) : "v"(mg[0]), "v"(min0));
                const int s0 = (signs ^ inp[1]) >> 31, s1 = (signs ^ inp[0]) >> 31;
                hout[0] = (o0 ^ s0) - s0;
                hout[1] = (o1 ^ s1) - s1;
                lds_wrx<TC>(ad[0], sat_sum_u8(inp[0], hout[0]));
                lds_wrx<TC>(ad[1], sat_sum_u8(inp[1], hout[1]));
            } else {
            int Lh[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) Lh[k] = lds_rdx<TC>(ad[k]);
            int xall = signs;
#pragma unroll
            for (int k = 0; k < NC; k++) {
                inp[k] = min(max(Lh[k] - hmb[k], -128), 127);
                mg[k] = mag_offset(Lh[k], hmb[k]);
                xall ^= inp[k];
            }
            int pre[NC + 1], suf[NC + 1]; // pre[k] = min(min0, mg[0..k)), suf[k] = min(mg[k..NC))
            pre[0] = min0; suf[NC] = 127;
#pragma unroll
            for (int k = 0; k < NC; k++) pre[k + 1] = min(pre[k], mg[k]);
#pragma unroll
            for (int k = NC - 1; k >= 0; k--) suf[k] = min(suf[k + 1], mg[k]);
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const int other = min(pre[k], suf[k + 1]);
                const int sg = (xall ^ inp[k]) >> 31;
                const int out = (other ^ sg) - sg;
                hout[k] = out;
                lds_wrx<TC>(ad[k], sat_sum_u8(inp[k], out));
            }
            }
        }
        // the next block reads what this one wrote: a workgroup barrier, unless both blocks sit inside one and the
        // same wavefront (LDS operations of a wave execute in program order)
        if ((start >> 6) != ((start + 2 * block - 1) >> 6)) lds_barrier();
    }
    if (!lane_chain || !(LR || DEG <= 20)) lds_barrier(); // (uniform; the last phase of a two-barrier lane chain and the outputs below touch different bits)
    DVBS2_PH(6); // ordered steps of the block scheme + closing barrier / completion of the chain rows
    if constexpr (V2P) {
        // LAST PHASE, packed: the ordered entries enter the packed domain as pairs [inp << 8] (what they read in their step is final), the
        // two smallest magnitudes are merged over everything, and every pair's outputs follow as in check_node_v2. The ordered entries'
        // LLRs were written in their step (a later row may have replaced them since): only their MESSAGES are produced here -- the same
        // "minimum and sign product over all other entries" the step computed, so the two agree by construction.
        if (work) {
            if constexpr (!KEEP_AD) v2p_addresses(NC);
            int m4[NC + 2];
            m4[0] = p0; m4[1] = p1;
#pragma unroll
            for (int j = 0; j < NPH; j++) {
                const uint32_t dh = __builtin_amdgcn_perm((uint32_t)inp[2 * j + 1], (uint32_t)inp[2 * j], 0x040c000cu); // [inp_hi << 8 | inp_lo << 8]
                dP[j] = as_v2s(dh);
                sxp ^= dh;
                aP[j] = __builtin_elementwise_max(dP[j], __builtin_elementwise_sub_sat(as_v2s(0u), dP[j]));
                m4[2 + 2 * j] = (int)(as_u32(aP[j]) & 0xffffu); m4[3 + 2 * j] = (int)(as_u32(aP[j]) >> 16);
            }
            int n0, n1;
            two_smallest<NC + 2>(m4, n0, n1);
            n0 &= 0x7f00; n1 &= 0x7f00;
            const int n0m = (int)__builtin_elementwise_sub_sat((uint32_t)n0, 256u), n1m = (int)__builtin_elementwise_sub_sat((uint32_t)n1, 256u);
            const int B0 = n0, B1 = n0 + n1m - n0m, T = n1m + n0;
            const v2s16 B0p = { (short)B0, (short)B0 }, B1p = { (short)B1, (short)B1 }, Tp = { (short)T, (short)T };
            const uint32_t tm = (uint32_t)((int)(sxp ^ (sxp << 16)) >> 31);
            uint32_t R[NP];
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int j = 0; j < NP; j++) {
                const v2s16 cl = __builtin_elementwise_min(__builtin_elementwise_max(aP[j], B0p), B1p);
                const v2s16 other = Tp - cl;
                const v2s16 sg = as_v2s(as_u32(dP[j]) ^ tm) >> (v2s16){ 15, 15 };
                const v2s16 out = as_v2s(as_u32(other) ^ as_u32(sg)) - sg;
                if (j >= NPH) {
                    const uint32_t nl = (as_u32(__builtin_elementwise_add_sat(dP[j], out)) ^ kObPair<TC>) >> 8;
                    lds_wr(ad[2 * j], (int)nl);
                    if (!(ODD && j == NP - 1)) lds_wr_hi(ad[2 * j + 1], nl);
                }
                R[j] = as_u32(__builtin_elementwise_min(__builtin_elementwise_max(out, (v2s16){ -32 * 256, -32 * 256 }), (v2s16){ 31 * 256, 31 * 256 }));
            }
            __builtin_amdgcn_s_setprio(3);
            if (ODD) R[NP - 1] &= 0x0000ffffu;
            msg_pack16<NP>(R, nm);
        }
        DVBS2_PH(7);
        return;
    }
    if constexpr (NC == 2) { mg[0] = clamp_mag(mg[0]); mg[1] = clamp_mag(mg[1]); } // raw in the loop (127 where no step ran: idle rows)
#pragma unroll
    for (int k = 0; k < NC; k++) {
        min1 = min(max(mg[k], min0), min1);
        min0 = min(min0, mg[k]);
        signs ^= inp[k];
        nm[k >> 2] |= (uint32_t)(min(max(hout[k], -32), 31) + 128) << (8 * (k & 3));
    }
    const int s01 = min0 + min1;
    if constexpr (LR) {
        // The regular entries only know the two smallest of THEMSELVES (p0, p1); after the ordered entries were merged a regular
        // entry's "minimum of the others" is: the entry that holds p0 takes min(second regular minimum, smallest ordered magnitude),
        // every other one min(first regular minimum, smallest ordered magnitude) -- i.e. min1 for the holder of the overall
        // minimum and min0 otherwise, decided on the merged (min0, min1) like this:
        //   hmin = smallest ordered magnitude (clamped); r0, r1 = the regular minima (clamped)
        //   holder of p0:  min(r1, hmin);   others:  min(r0, hmin)
        if (work) {
            int hmin = 127;
#pragma unroll
            for (int k = 0; k < NC; k++) hmin = min(hmin, mg[k]);
            const int o_first = min(pm_min_clamped(p1), hmin), o_rest = min(pm_min_clamped(p0), hmin);
#pragma unroll
            for (int k = NC; k < DEG; k++) {
                const int other = pm[k] == p0 ? o_first : o_rest;
                const int ip = pm_inp(pm[k]);
                const int sg = (signs ^ ip) >> 31;
                const int out = (other ^ sg) - sg;
                const int nl = sat_sum_u8(ip, out);
                if (!(LAYER0 && k == DEG - 1) || last_valid) lds_wrx<TC>(addr(k), nl);
                nm[k >> 2] |= (uint32_t)(min(max(out, -32), 31) + 128) << (8 * (k & 3));
            }
        }
    } else
    if (work) {
#pragma unroll
        for (int k = 0; k < DEG; k++) {
            if (k >= NC) {
                const int other = s01 - vmed3_i32(mg[k], min0, min1); // regular entries hold raw magnitudes
                const int sg = (signs ^ inp[k]) >> 31;
                const int out = (other ^ sg) - sg;
                const int nl = sat_sum_u8(inp[k], out);
                if (OWN_REG && k == DEG - 2) *carry = nl;
                else if (PREV_REG && k == DEG - 1) spare = nl;
                else if (!(LAYER0 && k == DEG - 1) || last_valid) lds_wrx<TC>(ad[k], nl);
                nm[k >> 2] |= (uint32_t)(min(max(out, -32), 31) + 128) << (8 * (k & 3));
            }
        }
        if (PR) nm[1] = (nm[1] & 0x00ffffffu) | ((uint32_t)spare << 24);
    }
    DVBS2_PH(7); // merge + outputs of the regular entries
#undef DVBS2_PH
}

} // namespace dvbs2
