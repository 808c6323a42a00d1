// ldpc_kernel.hpp -- the sweep kernel of the layered LDPC decoder: the dispatch of a layer to the check node of its degree and kind,
// the full syndrome test's sign vectors and ldpc_layered_kernel itself. Included through ldpc_inst.hpp by the per-variant translation units
// ldpc_inst_*.hip, which instantiate one DMAX each so that the kernel variants compile in parallel. The host sees ldpc_launch.h only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "demap_math.hpp"
#include "ldpc_launch.h"
#include "ldpc_prims.hpp"
#include "ldpc_node_plain.hpp"
#include "ldpc_node_packed.hpp"
#include "ldpc_node_hazard.hpp"

namespace dvbs2 {

// degrees DMAX-7 .. DMAX are instantiated for kernel variant DMAX
#define DVBS2_DEG_CASE(D) case D: if constexpr (D >= 3 && D <= DMAX && D > DMAX - 8) { \
        { if (layer0) check_node<(D >= 3 ? D : 3), true, false, false, TC>(lds_all, ent, jj, lb, mw, nm); else { if constexpr (!kPure) check_node<(D >= 3 ? D : 3), false, false, false, TC>(lds_all, ent, jj, lb, mw, nm); } } } else DVBS2_NM_CLEAR break;
#define DVBS2_DEG_SWITCH switch (deg) { DVBS2_DEGREES_3_32(DVBS2_DEG_CASE) default: DVBS2_NM_CLEAR break; }

#define DVBS2_V2_CASE(D) case D: if constexpr (D >= 3 && D <= DMAX && D > DMAX - 8) { check_node_v2<(D >= 3 ? D : 3), DMAX, TC>(ent, jj + lb, mw, nm, prefetch); } else DVBS2_NM_CLEAR break;
#define DVBS2_V2_SWITCH switch (deg) { DVBS2_DEGREES_3_32(DVBS2_V2_CASE) default: DVBS2_NM_CLEAR break; }
// (a degree the build does not instantiate -- a case without a body, or the default -- never occurs in a record. Left undefined there, nm became a value carried round the
// layer loop: one 64-bit register copy per layer on EVERY path. Defined there, it costs the paths that run nothing.)
#define DVBS2_NM_CLEAR { _Pragma("unroll") for (int w_ = 0; w_ < MW; w_++) nm[w_] = 0u; }
// the run loop of the degree classes up to 8 (kRun in the kernel): one dispatch per RUN of regular packed layers, on the header's count field
#define DVBS2_RUN_CASE(D) case D - 2: if constexpr (D >= 3 && D <= DMAX && D > DMAX - 8) { run(std::integral_constant<int, (D >= 3 ? D : 3)>{}); } break;

#define DVBS2_CHAIN_CASE(D) case D: if constexpr (D >= 4 && D <= DMAX && D > DMAX - 8) { check_node_chain_v2<(D >= 4 ? D : 4), DMAX, TC>(ent, jj, jj + lb, work, block, mw, nm, htab16, hb_ctr, hb_epoch, hb_lane); } break;
#define DVBS2_CHAIN_SWITCH switch (deg) { DVBS2_DEGREES_4_32(DVBS2_CHAIN_CASE) default: break; }

// check_node_hazard with its switches given by name (HazardCfg, ldpc_node_hazard.hpp): what this build fixes, then what the call adds
#define DVBS2_HAZ_NODE(D, NCV, ...) \
        check_node_hazard<D, NCV, HazardCfg<hz::two_level<HZ2>, hz::chain_ok<(MINW == 1)>, hz::class8<(DMAX <= 8)>, hz::tc<TC>, __VA_ARGS__>>( \
            lds_all, ent, jj, lb, work, block, block2, mw, nm, 0, nullptr, htab, hb_ctr, hb_epoch, hb_lane, hz_ph);
// (A layer that runs the two-level lane chain gets an instantiation of its own -- TLC and the low-register form, which keeps one
// word per regular entry across the outer blocks instead of three --: compiled into the common instantiation the chain's register
// state made the compiler spill the regular entries of EVERY four- and eight-entry layer around it, 9/10 normal's multi-pair
// layers went from 12-17 k to 25-34 k cycles.)
#define DVBS2_HAZ_CALL1(D, NCV, LRV, TLCV) { \
        if (layer0) DVBS2_HAZ_NODE(D, NCV, hz::layer0<true>, hz::low_reg<LRV>, hz::tlc<TLCV>) \
        else { if constexpr (!kPure) DVBS2_HAZ_NODE(D, NCV, hz::layer0<false>, hz::low_reg<LRV>, hz::tlc<TLCV>) } }
#define DVBS2_HAZ_CALL(D, NCV) { if constexpr (D - 2 >= NCV) { \
        if constexpr (kTlc<DMAX, HZ2> && !SOFT && MINW == 1 && (NCV == 4 || NCV == 8)) { if (block2 > 0 && htab != nullptr) DVBS2_HAZ_CALL1(D, NCV, (DMAX >= kTlcLowRegMinDmax), true) else DVBS2_HAZ_CALL1(D, NCV, false, false) } \
        else DVBS2_HAZ_CALL1(D, NCV, false, false) } }
#define DVBS2_HAZ_CASE(D) case D: if constexpr (D >= 4 && D <= DMAX && D > DMAX - 8) { \
        if (nc == 2) DVBS2_HAZ_CALL((D >= 4 ? D : 4), 2) else if (nc == 4) DVBS2_HAZ_CALL((D >= 4 ? D : 4), 4) else { if constexpr (HZ2 && DMAX <= kMaxHazard12Dmax) { if (nc == 8) DVBS2_HAZ_CALL((D >= 4 ? D : 4), 8) else DVBS2_HAZ_CALL((D >= 4 ? D : 4), 12) } else DVBS2_HAZ_CALL((D >= 4 ? D : 4), 8) } } break;
// The same with the packed first / last phase (packed_phases): regular layers i > 0 of the builds with packed nodes whose
// wave record the host laid out in the packed format (header bit 14); the ordered phase is the plain one, instantiation for instantiation.
#define DVBS2_HAZP_CALL1(D, NCV, TLCV) { DVBS2_HAZ_NODE(D, NCV, hz::tlc<TLCV>, hz::packed_phases<true>, hz::dmaxv<DMAX>) }
#define DVBS2_HAZP_CALL(D, NCV) { if constexpr (D - 2 >= NCV) { \
        if constexpr (kTlc<DMAX, HZ2> && !SOFT && MINW == 1 && (NCV == 4 || NCV == 8)) { if (block2 > 0 && htab != nullptr) DVBS2_HAZP_CALL1(D, NCV, true) else DVBS2_HAZP_CALL1(D, NCV, false) } \
        else DVBS2_HAZP_CALL1(D, NCV, false) } }
#define DVBS2_HAZP_CASE(D) case D: if constexpr (D >= 4 && D <= DMAX && D > DMAX - 8) { \
        if (nc == 2) DVBS2_HAZP_CALL((D >= 4 ? D : 4), 2) else if (nc == 4) DVBS2_HAZP_CALL((D >= 4 ? D : 4), 4) else DVBS2_HAZP_CALL((D >= 4 ? D : 4), 8) } break;
#define DVBS2_HAZP_SWITCH switch (deg) { DVBS2_DEGREES_4_32(DVBS2_HAZP_CASE) default: break; }
#define DVBS2_HAZ_SWITCH switch (deg) { DVBS2_DEGREES_4_32(DVBS2_HAZ_CASE) default: break; }

// Step 1 of the full syndrome test (see the kernel): the 360-bit sign vectors of all N / 360 groups, one thread per eight consecutive
// LLR bytes; returns non-zero when one of this thread's bytes is a zero LLR. A function of its own, NOT inlined: inlined, its loop
// perturbed the register allocation of the sweep and cost the never-converging batches -- where it never runs -- up to 4 % (S2X 154/180).
__device__ __attribute__((noinline)) int syndrome_sign_vectors(const lds_byte_t* lds, lds_u32_t* sv, int N, int tid, bool tc /*LLR bytes are two's complement*/)
{
    lds_byte_t* svb = reinterpret_cast<lds_byte_t*>(sv);
    int zero = 0;
#pragma unroll 2
    for (int blk = tid; blk < N / 8; blk += kHalf) {
        const v2u32 v = *reinterpret_cast<const lds_v2u_t*>(lds + 8 * blk);
        const uint32_t ob = tc ? 0u : 0x80808080u;
        const uint32_t xa = v.x ^ ob, xb = v.y ^ ob; // two's complement: zero bytes = zero LLRs
        zero |= (int)((((xa - 0x01010101u) & ~xa) | ((xb - 0x01010101u) & ~xb)) & 0x80808080u);
        // sign bit of byte i -> bit i (offset binary: negative <=> bit 7 clear): bits 0, 8, 16, 24 gathered by a multiply
        const uint32_t na = (((xa & 0x80808080u) >> 7) * 0x01020408u) >> 24, nb = (((xb & 0x80808080u) >> 7) * 0x01020408u) >> 24;
        const int g = blk / 45;
        svb[g * (kSvWords * 4) + (blk - 45 * g)] = (uint8_t)((na & 0xfu) | ((nb & 0xfu) << 4));
    }
    return zero;
}

constexpr int kSoloThreads = 512;
static_assert(kCuSlots == 16 * 8 * 2 * 16, "the per-CU counter table (ldpc_layout.h) must hold every index hw_cu_index() can return: XCC x SE x SH x CU");
__device__ __forceinline__ uint32_t hw_cu_index()
{
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    // HW_ID: simd_id[5:4] cu_id[11:8] sh_id[12] se_id[15:13]
    return ((((xcc & 0xfu) * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u + ((hw >> 8) & 0xfu));
}

// MINW = 6 ("dense"): compiled for 80 VGPRs so that two pair-workgroups share a CU when the frames are short enough for
// LDS. It spills and only pays where ordered hazard steps dominate (ldpc_plan.cpp picks it).
// V2: the packed nodes (check_node_v2, check_node_chain_v2) are compiled in; a table runs the build that measured faster for it
// (compiling both families into one kernel costs each of them 4-7 % through register allocation).
// SOLO: ONE frame per workgroup, two (or more) independent workgroups per CU. The pair workgroup exists only to put three
// waves on every SIMD; its price is that the hardware barrier couples the two frames, so each one also waits through the other's
// ordered hazard steps, LDS round trips and stragglers. Two separate 6-wave workgroups land 4,2,3,3 on the SIMDs
// (tools/ubench/placement.hip: waves go round the SIMDs, the next workgroup starts one position later). SOLO launches EIGHT waves
// -- always two per SIMD -- and lets two of them leave at once: a workgroup keeps both waves on one pair of SIMDs and one
// wave on the other pair, and workgroups sharing a CU take complementary patterns (a counter pair per CU in global memory).
// Result: three working waves per SIMD again, but the frames no longer wait for each other. Needs <= 128 VGPRs.
template <int DMAX, bool TIMING, int MINW = 1, bool V2 = false, bool SOLO = false, bool HZ2 = false, bool SOFT = false /*SOFT: frame barriers in software -- a build of its own: the barrier state in every barrier of
                             every build cost the 80-VGPR build 25-30 % (54 -> 199 spilled VGPRs) and the degree classes 20..32 4-10 %*/
          /*HZ2: heavy hazard layers: twelve ordered entries, two-level walk (check_node_hazard); a build of its own because the
                             extra register state costs the degree classes 28 and 32 ten percent everywhere else (B11, S2X B21)*/>
__global__ __launch_bounds__(SOLO ? kSoloThreads : kThreads, SOLO ? 4 : MINW) void ldpc_layered_kernel(
    const uint32_t* __restrict__ recs, const uint32_t* __restrict__ wrecs /*per (layer, wave) sweep records*/,
    const int8_t* __restrict__ llr_in, uint8_t* __restrict__ state,
    uint32_t* __restrict__ msgs, int* __restrict__ iters, int* __restrict__ good, const int* __restrict__ target,
    int n_frames, int N, int K, int q, int cap, int stop_on_good /*bit 0: stop at a good syndrome, bit 1: software frame barriers, bit 2: group-synchronous stop*/,
    unsigned long long* __restrict__ tdbg, int* __restrict__ cu_slots,
    const DemapFused dm /*mode != 0: a fresh decode takes XFECFRAME symbols and demaps while loading (llr_in is null then)*/)
{
    unsigned long long tm_bar = 0, tm_body = 0, tm_conf = 0, tm_synd = 0, tm_sweep = 0, tm_load = 0, tm_s1 = 0;
#define TSTAMP(x) do { if (TIMING) { x = __builtin_readcyclecounter(); } } while (0)
    unsigned long long tA = 0, tB = 0, tC = 0, tS0 = 0, tS1 = 0;
    const bool fresh = llr_in != nullptr || dm.mode != 0;
    if (!fresh) { // resume launch: a workgroup whose frames are all at their target leaves before touching LDS
        const int fa = SOLO ? (int)blockIdx.x : 2 * (int)blockIdx.x, fb = SOLO ? fa : fa + 1;
        const bool ta = fa < n_frames && iters[fa] < target[fa];
        const bool tb = fb < n_frames && iters[fb] < target[fb];
        if (!ta && !tb) return;
    }
    TSTAMP(tA);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_all[];
    constexpr int RS = rec_stride(DMAX);
    constexpr int RSW = V2 ? 6 * rec_stride_wave(DMAX) : rec_stride(DMAX); // dwords from one layer's sweep record to the next
    constexpr int MW = DMAX / 4; // message dwords per check (fixed per kernel variant)
    // "pure" packed builds (v2_pure_class): the plain nodes are compiled for layer 0 only -- the plain hazard
    // nodes of the degree class 32 cost the packed ones around them 5 % through register allocation --; the host runs such a build only
    // for tables whose every (layer > 0, wave) record fits the packed format (ldpc_plan.cpp)
    // (also the software-barrier packed build of the pure classes: S2X 154/180 131.8 -> 133.9 k with ten fix slots, round 5)
    constexpr bool kPure = V2 && v2_pure_class(DMAX);
    constexpr bool TC = V2 && DMAX <= kTcMaxDmax;        // LLR bytes in LDS as two's complement (see lds_rdx)
    constexpr uint32_t kObState = TC ? 0x80808080u : 0u;        // LDS bytes <-> the offset-binary state in HBM
    int solo_tid = (int)threadIdx.x;
    int solo_slot = -1, solo_pat = 0;
    if constexpr (SOLO) {
        // role election (the first words of LDS are scratch until the LLRs are loaded)
        volatile lds_i32_t* e = reinterpret_cast<volatile lds_i32_t*>((lds_byte_t*)lds_all); // [0..3] waves seen per SIMD, [4] workers so far, [5] pattern
        if (threadIdx.x < 8) e[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x == 0) {
            solo_slot = (int)hw_cu_index();
            int* w = cu_slots + solo_slot; // low half: workgroups with pattern 0 resident on this CU, high half: pattern 1
            int old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), pat;
            do { pat = (old & 0xffff) <= (old >> 16) ? 0 : 1; }
            while (!__hip_atomic_compare_exchange_strong(w, &old, old + (pat ? 0x10000 : 1), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            e[5] = pat; e[6] = solo_slot;
        }
        __syncthreads();
        solo_pat = e[5]; solo_slot = e[6];
        int widx = -1;
        if ((threadIdx.x & 63) == 0) {
            uint32_t hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            const int simd = (int)((hw >> 4) & 3u);
            const int rank = __hip_atomic_fetch_add(const_cast<lds_i32_t*>(e) + simd, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const bool two = ((simd >> 1) & 1) == solo_pat; // pattern 0 keeps both waves on SIMDs 0,1; pattern 1 on SIMDs 2,3
            if (two || rank == 0) widx = __hip_atomic_fetch_add(const_cast<lds_i32_t*>(e) + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        widx = __builtin_amdgcn_readfirstlane(widx);
        __syncthreads();
        // a workgroup that was NOT placed two waves per SIMD elects fewer or more than six: the surplus leaves, a shortfall cannot
        // be repaired (it has not been observed; the launch would then miss rows) -- so insist on six by falling back to arrival order
        const int nworkers = e[4];
        if (nworkers != 6) widx = (int)(threadIdx.x >> 6) < 6 ? (int)(threadIdx.x >> 6) : -1;
        __syncthreads(); // everyone has read the election words; they may be overwritten now
        if (widx < 0 || widx >= 6) return; // the two spare waves leave (the hardware barrier no longer counts them)
        solo_tid = widx * 64 + (int)(threadIdx.x & 63);
    }
    const int half = SOLO ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >= kHalf ? 1 : 0); // wave-uniform, and the compiler knows it
    const int tid = SOLO ? solo_tid : (int)threadIdx.x - half * kHalf;
    const int lb_rel = half * (int)half_lds_bytes(N);
    const int lb = lb_rel + lds_address_of(lds_all); // absolute LDS address of this frame's region
    lds_byte_t* lds = (lds_byte_t*)lds_all + lb_rel; // (typed pointers: see lds_byte_t)
    lds_u32_t* sv = reinterpret_cast<lds_u32_t*>(lds + N); // N % 8 == 0
    volatile lds_i32_t* flags = reinterpret_cast<volatile lds_i32_t*>(sv + sv_area_words(N)); // [0] bad-or, [1] finished, [2] pre-test failed, [3] full test needed
    volatile lds_i32_t* other_flags = reinterpret_cast<volatile lds_i32_t*>(
        (lds_byte_t*)lds_all + (1 - half) * (int)half_lds_bytes(N) + N + sv_area_words(N) * 4);
    const int f = SOLO ? (int)blockIdx.x : 2 * (int)blockIdx.x + half;
    const bool have_frame = f < n_frames;
    const int lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave); // the same value, known to be uniform (scalar addressing of the records)
    const int NG = N / kM;
    const bool active = tid < kM;

    int it = 0, tgt = 0;
    bool finished = !have_frame; // this half has nothing (more) to do; it still takes part in every barrier
    if (have_frame) {
        tgt = target ? target[f] : cap;
        if (fresh && dm.mode != 0) {
            // demapper fused into the load: symbol s gives LLRs 2 s, 2 s + 1 (QPSK, natural order) or the three column positions
            // ra0 + s, ra1 + s, ra2 + s (8PSK de-interleaver), each stored at its place of the internal layout
            auto put = [&](int n, int8_t v) {
                int idx = n;
                if (n >= K) { const int r = n - K, jq = r / q; idx = K + kM * (r - jq * q) + jq; } // pty[360*i + j] = parity[q*j + i]
                lds[idx] = (uint8_t)v ^ (TC ? 0x00u : 0x80u);
            };
            const float N0 = dm.n0[dm.n0_count > 1 ? f : 0];
            const float2* src = reinterpret_cast<const float2*>(dm.syms) + (size_t)f * dm.n_syms;
            if (dm.mode == 1) {
                const float scalar = qpsk_scalar(N0);
                for (int sidx = tid; sidx < dm.n_syms; sidx += kHalf) {
                    const float2 v = src[sidx];
                    put(2 * sidx, qpsk_llr(v.x, scalar)); put(2 * sidx + 1, qpsk_llr(v.y, scalar));
                }
            } else {
                const float dp = psk8_dist_prec(N0);
                for (int sidx = tid; sidx < dm.n_syms; sidx += kHalf) {
                    const float2 v = src[sidx];
                    int8_t b0, b1, b2;
                    psk8_llr(v.x, v.y, dm.rr, dm.ri, dp, b0, b1, b2);
                    put(dm.ra0 + sidx, b0); put(dm.ra1 + sidx, b1); put(dm.ra2 + sidx, b2);
                }
            }
        } else if (fresh) {
            const uint2* src = reinterpret_cast<const uint2*>(llr_in + (size_t)f * N);
            for (int c = tid; c < N / 8; c += kHalf) {
                uint2 v = src[c];
                if constexpr (!TC) { v.x ^= 0x80808080u; v.y ^= 0x80808080u; }
                const int n = 8 * c;
                if (n < K) *reinterpret_cast<lds_v2u_t*>(lds + n) = (v2u32){ v.x, v.y }; // K % 8 == 0
                else {
                    // pty[360*i + j] = parity[q*j + i] (layered_decoder.hh:150-152)
                    int r = n - K;
                    int jq = r / q, iq = r - jq * q;
#pragma unroll
                    for (int b = 0; b < 8; b++) {
                        lds[K + kM * iq + jq] = (uint8_t)((b < 4 ? v.x >> (8 * b) : v.y >> (8 * (b - 4))) & 0xffu);
                        if (++iq == q) { iq = 0; ++jq; }
                    }
                }
            }
        } else {
            it = iters[f];
            if (it >= tgt) finished = true; // nothing to do for this frame in this pass
            else {
                const uint2* src = reinterpret_cast<const uint2*>(state + (size_t)f * N);
                for (int c = tid; c < N / 8; c += kHalf) { const uint2 v = src[c]; *reinterpret_cast<lds_v2u_t*>(lds + 8 * c) = (v2u32){ v.x ^ kObState, v.y ^ kObState }; } // (the state in HBM is offset binary in every build)
            }
        }
    }
    const bool untouched = finished; // never loaded: must not write state/iters/good back
    if (tid == 0) { flags[0] = 0; flags[2] = 0; flags[3] = 0; flags[1] = finished ? 1 : 0; flags[4] = 0; }
    // Frame barriers in software (bit 1 of the flag word; pair workgroups only): worth it for high-degree tables without hazard
    // layers -- few barriers, long layers: S2X B21 +12 %, S2X B10 +10 % -- and a loss where barriers are frequent (B4 -8 %: the
    // counter costs ~300 cycles per barrier against ~30 for s_barrier). Chosen per table by the host.
    constexpr bool soft_bar = SOFT; // (bit 1 of the flag word is what the host sets when it launches this build)
    volatile lds_i32_t* hb_ctr = soft_bar ? flags + 4 : nullptr; // frame barrier counter (frame_barrier)
    int hb_epoch = 0;
    const int hb_lane = lane;
    __syncthreads();
    TSTAMP(tB); tm_load = tB - tA;

    // Messages go through a buffer descriptor based at this frame's records: the per-lane offset (the row's, rm = row * kMsgRowBytes) is
    // loop-invariant and the per-layer offset (plus the word's) is a scalar operand, so a message access costs no
    // VALU address arithmetic (a flat 64-bit address costs two to four VALU instructions per access).
    // Layout: ldpc_layout.h (msg_row_bytes). With two words per check a row's record is loaded and stored with ONE 8-byte access.
    uint32_t* msg_base = msgs + (size_t)(have_frame ? f : 0) * q * MW * kMsgStride;
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(msg_base, 0, q * MW * kMsgStride * 4, 0x00020000);
    constexpr int kLayerBytes = MW * kMsgStride * 4;
    constexpr int kMsgRowBytes = msg_row_bytes(MW), kMsgWordStep = msg_word_step(MW);
#define MSG_LD(soff, w, rm) __builtin_amdgcn_raw_buffer_load_b32(mrs, (rm), (soff) + (w) * kMsgWordStep, 0)
#define MSG_ST(v, soff, w, rm) __builtin_amdgcn_raw_buffer_store_b32((v), mrs, (rm), (soff) + (w) * kMsgWordStep, 0)
    auto msg_load = [&](uint32_t* dst, int soff, int rm) {
        if constexpr (MW == 2) {
            const v2u32 v = __builtin_amdgcn_raw_buffer_load_b64(mrs, rm, soff, 0);
            dst[0] = v.x; dst[1] = v.y;
        } else {
#pragma unroll
            for (int w = 0; w < MW; w++) dst[w] = MSG_LD(soff, w, rm);
        }
    };
    auto msg_store = [&](const uint32_t* src, int soff, int rm) {
        if constexpr (MW == 2) {
            __builtin_amdgcn_raw_buffer_store_b64((v2u32){ src[0], src[1] }, mrs, rm, soff, 0);
        } else {
#pragma unroll
            for (int w = 0; w < MW; w++) MSG_ST(src[w], soff, w, rm);
        }
    };
    // The messages of the layer at hand (mw <- pre) and the load of the next layer's (byte offset `next`) into pre. In a frame's first sweep
    // (zero) nothing is loaded and mw is the zero message of the layer's format. The first-sweep arm is a real branch (the empty asm
    // statement cannot be speculated, so the arm is not turned into selects), and the load is unconditional in every other sweep -- the
    // last layer fetches layer 0's record again, whose store is 89 layers and as many vmcnt(0) waits old, and drops it --: with a load
    // that may not happen the old pre had to survive it, which cost a second 64-bit copy per layer.
    auto take_msgs = [&](uint32_t* mw, uint32_t* pre, bool zero, uint32_t zero_word, int next, int rm) {
#pragma unroll
        for (int w = 0; w < MW; w++) mw[w] = pre[w];
        if (zero) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int w = 0; w < MW; w++) mw[w] = zero_word;
        } else msg_load(pre, next, rm);
    };
    // bnl = 0 before the first update (layered_decoder.hh:27-31,149): a frame's first sweep (it == 0, in the first pass or
    // when a frame that stopped at once is resumed) takes offset-binary zero bytes instead of loading them -- no memset
    // of the record area, no read traffic in sweep 0
    bool is_good = false;

    for (;;) {
        TSTAMP(tS0);
        // ---- syndrome test (layered_decoder.hh:32-49, algorithms.hh:195-202): bad if any check has a zero
        // LLR or an odd number of negative LLRs. Barriers are taken by every thread; work only by halves that need it.
        const bool need_synd = !finished && ((stop_on_good & 1) || it >= tgt);
        // Pre-test (the reference's bad() also returns at the first failing check): the 360 checks of ONE layer,
        // tested edge by edge. A failure here is final; only a frame that passes pays for the full test below.
        // (Round 4 measured a "sticky" choice of the pre-tested layer -- the layer in which the last full test found an unsatisfied check
        // instead of `it mod q`, so that a nearly converged frame skips full tests: exact, and no measurable change at the operating point
        // of bench.py (282.8 k vs 282.9 k frames/s): the full test is ~3 % of an update in which it runs. Not kept.)
        if (need_synd && active) {
            const int i0 = it % q;
            const uint32_t* rec = recs + (size_t)i0 * RS;
            const int deg = (int)(rec[0] & 0xffu) + 2;
            uint32_t x = 0, z = 0;
            // per build, measured (round 6, interleaved A/B of whole tables against the edge-by-edge loop): 9/10 normal +4.7 %, 5/6 +4.0 %, 8/9 +2.0 %,
            // 4/5 +1.3 %, S2X 25/36 +1.6 %, 1/4 normal +1.0 %, short 3/5 (the 80-VGPR build) +45 %; 3/4 normal -2.5 % and short 2/3 -1.0 % (class 16),
            // S2X 154/180 -1.8 % (class 32 with software barriers), B4 and short 1/4 unchanged
            constexpr bool kPretestChunk = DMAX != 16 && !(DMAX == 32 && SOFT);
            if constexpr (kPretestChunk) {
            // Round 6: FOUR edges per trip -- their eight record words in one scalar load, the four LDS reads in flight together. Edge by
            // edge the loop paid one scalar-cache round trip and one LDS round trip per edge (~300 cycles x 30 edges of a 9/10 normal
            // check: the syndrome phase was 19 k of its 342 k cycles per update, cycle stamps). (records are padded to DMAX entries,
            // DMAX is a multiple of four: the last trip never reads past its record; an edge past the degree reads byte `tid` and is ignored)
            for (int k0 = 0; k0 < deg; k0 += 4) {
                uint32_t e[8], v[4];
#pragma unroll
                for (int u = 0; u < 8; u++) e[u] = rec[4 + 2 * k0 + u];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int a0 = tid + (int)e[2 * u] - ((uint32_t)tid < e[2 * u + 1] ? 0 : kM);
                    v[u] = (uint32_t)lds[k0 + u < deg ? a0 : tid];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    uint32_t w = v[u] ^ (TC ? 0x80u : 0x00u); // offset-binary value
                    if (i0 == 0 && k0 + u == deg - 1 && tid == 0) w = 0x81u; // check (0,0) has no previous parity: neutral +1
                    if (k0 + u < deg) { x ^= w; z |= (w == 0x80u); }
                }
            }
            } else
            for (int k = 0; k < deg; k++) {
                const int a0 = tid + (int)rec[4 + 2 * k] - ((uint32_t)tid < rec[5 + 2 * k] ? 0 : kM);
                uint32_t v = (uint32_t)lds[a0] ^ (TC ? 0x80u : 0x00u); // offset-binary value
                if (i0 == 0 && k == deg - 1 && tid == 0) v = 0x81u; // check (0,0) has no previous parity: neutral +1
                x ^= v;
                z |= (v == 0x80u);
            }
            // offset binary: the sign bit is inverted, so the count of negatives is deg - popcount(bit 7)
            const int bad_pre = (int)((((x >> 7) ^ (uint32_t)deg) & 1u) | z);
            if (__ballot(bad_pre) != 0 && lane == 0) flags[2] = 1;
        }
        lds_barrier();
        const bool need_full = need_synd && flags[2] == 0;
        if (tid == 0) flags[3] = need_full ? 1 : 0;
        lds_barrier();
        const bool full_any = flags[3] != 0 || (!soft_bar && !SOLO && other_flags[3] != 0); // uniform over the barrier domain
        if (full_any) {
        if (need_full) {
            // Step 1: 360-bit sign vector per group. Round 3: one thread per EIGHT consecutive LLR bytes (one 8-byte LDS read -> one
            // byte of the vector: 360 = 45 x 8, so a block never straddles two groups) instead of one byte read and two ballots per
            // thread and group -- a fifth of the LDS instructions; at the operating point, where nearly every test is a full one,
            // the tests were a tenth of the decode (cycle stamps).
            {
                const int zero = syndrome_sign_vectors(lds, sv, N, tid, TC);
                if (__ballot(zero != 0) != 0 && lane == 0) flags[0] = 1;
            }
        }
        TSTAMP(tC); tm_s1 += tC - tS0;
        lds_barrier();
        if (need_full && tid < NG) { // wrap extension: bits 360+u = bit u
            lds_u32_t* p = sv + tid * kSvWords;
            const uint32_t w0 = p[0], w1 = p[1];
            p[11] = (p[11] & 0xffu) | (w0 << 8);
            p[12] = (w0 >> 24) | (w1 << 8);
        }
        lds_barrier();
        if (need_full) {
            // Step 2: parity word (layer i, lanes 32w..32w+31) = xor over entries of the rotated sign vectors
            // (this one stays inline: as a function of its own its record arrays made the degree classes 12-dense and 32 two to
            // three times slower -- the kernel then has to provide the callee's registers on top of its own)
            int bad = 0;
            for (int item = tid; item < q * 12; item += kHalf) {
                const int i = item / 12, w = item - 12 * i;
                const uint32_t* rec = recs + (size_t)i * RS;
                const int deg = (int)(rec[0] & 0xffu) + 2;
                uint32_t e0[DMAX], e1[DMAX];
#pragma unroll
                for (int k = 0; k < DMAX; k++) { e0[k] = rec[4 + 2 * k]; e1[k] = rec[5 + 2 * k]; } // padded records: always readable
                uint32_t acc = 0;
#pragma unroll
                for (int k = 0; k < DMAX; k++) {
                    if (k < deg) {
                        const int rot = kM - (int)e1[k];   // S0 = 360*g + rot, thr = 360 - rot
                        const int g360 = (int)e0[k] - rot;
                        const int t0 = wrap360(32 * w + rot);
                        const lds_u32_t* p = sv + (g360 / kM) * kSvWords + (t0 >> 5);
                        uint32_t x = __funnelshift_r(p[0], p[1], t0 & 31);
                        if (i == 0 && k == deg - 1 && w == 0) x &= ~1u; // check (0,0): no previous parity
                        acc ^= x;
                    }
                }
                if (w == 11) acc &= 0xffu;
                bad |= acc != 0;
            }
            if (__ballot(bad) != 0 && lane == 0) flags[0] = 1;
        }
        lds_barrier();
        } // full_any
        if (need_synd) is_good = need_full && flags[0] == 0;
        const bool gs = (stop_on_good & 5) == 5; // group-synchronous stop (group_decide), first pass only
        if (!finished && (it >= tgt || (!gs && (stop_on_good & 1) && is_good))) finished = true;
        lds_barrier(); // everyone has read flags[0]
        if (wave_u == 0) { // (the whole first wave: group_decide reads one status word per lane)
            int fin = finished ? 1 : 0;
            if (gs && !finished) {
                const uint32_t* hd = recs - kRecHeaderWords; // (uniform: scalar loads)
                const int* iters0 = reinterpret_cast<const int*>(((unsigned long long)hd[1] << 32) | hd[0]);
                int* status = reinterpret_cast<int*>(((unsigned long long)hd[3] << 32) | hd[2]);
                const int G = (int)hd[4];
                const int g = f / G; // within this launch (its first frame is a multiple of the group size)
                fin = group_decide(status + (iters - iters0) + g * G, min(G, n_frames - g * G), f - g * G, it, is_good, lane, (int)hd[5]) != 0;
            }
            if (tid == 0) { flags[0] = 0; flags[2] = 0; flags[1] = fin; }
        }
        lds_only_barrier();
        if (gs) finished = flags[1] != 0; // (uniform over the frame)
        TSTAMP(tS1); tm_synd += tS1 - tS0;
        if (finished && (soft_bar || SOLO || other_flags[1])) break; // uniform over the barrier domain

        // ---- one update sweep: layered_decoder.hh:50-79 ----
        // Threads 360..383 of a half mirror check row 359: same reads, same results, same (duplicate) writes. That
        // keeps the whole sweep free of per-lane predicates: `work` is wave-uniform.
        const bool work = __builtin_amdgcn_readfirstlane(finished ? 0 : 1) != 0; // uniform over the wave, and the compiler knows it
        const int row = tid < kM ? tid : kM - 1;
        const int rowm = row * kMsgRowBytes; // this row's byte offset in a layer's message records
        // uniform over the half, and the compiler knows it: the zero messages of a frame's first sweep are a scalar branch per layer
        // (take_msgs), not a compare mask and one v_cndmask per message word in every layer of every sweep
        const bool zero_msgs = __builtin_amdgcn_readfirstlane(it) == 0;
        // timing builds: cycles per phase of the hazard nodes, frame 0, lane 0 of waves 0 and 5 (slots 256.. and 272.. after the per-layer sums)
        unsigned long long* const hz_ph = (TIMING && tdbg && f == 0 && (tid == 0 || tid == 320)) ? tdbg + (size_t)n_frames * 48 + 256 + (tid ? 16 : 0) : nullptr;
        uint32_t pre[MW]; // messages of the next layer for check tid, loaded one layer ahead
        constexpr bool kWaitStore = !SOFT; // (DVBS2_WAIT_VM0)
        if (work) {
#pragma unroll
            for (int w = 0; w < MW; w++) {
                pre[w] = zero_msgs ? 0x80808080u : MSG_LD(0, w, rowm);
            }
        }
        // Layer records are double-buffered in SGPRs: the scalar loads of layer i+1 are issued at the top of layer i
        // (an un-prefetched s_load at the head of every layer was a quarter of the sweep time). Small records are
        // buffered whole; for the large ones only every 8th dword is carried over -- enough to pull each cache
        // line of the next record into the scalar cache -- and the rest is loaded at the top of the layer.
        // (Rounds 1-3 carried every 8th word of the large records over from the previous layer; round 4 measured none -- the header words only --
        // 1-9 % faster on 16 of 17 tables of the classes 16-32: each carried word was its own `s_load_dword; s_waitcnt lgkmcnt(0); v_writelane`
        // at every layer head, and the records of a table (5-7 KB) stay in the scalar cache anyway.)
        // Up to kPfSmallMaxDmax the whole record is double-buffered in scalar registers. Measured: class 8 loses 2-3 % without it
        // (B4 119.7 -> 117.1 k), class 12 GAINS 1-3 % without it (3/5, 2/3 normal, S2X 11/20, T2 2/3, short 2/3; short 3/5 -0.7 %)
        // Run loop: the packed builds of the degree classes up to 8 run their regular packed layers in a loop of their own (at the head
        // of the layer loop). At three waves per SIMD a wave is limited by its own instruction stream, scalar instructions included, and
        // the layer loop spent 67 of them per regular trip on the record double buffer's moves, the header decode and the degree switch as
        // a compare chain -- for a degree and a record format that change nine times in B4's 90 layers (notes/r09_run_loop.md, r10_straight_trip.md).
        constexpr bool kRun = V2 && DMAX <= 8;
        constexpr int kPfSmallMaxDmax = 8;
        constexpr int PF = DMAX <= kPfSmallMaxDmax ? 1 : 2 * DMAX;
        static_assert(!kRun || PF == 1, "the run loop takes over whole records fetched ahead into scalar registers");
        // the sweep reads the records of its own WAVE (check_node_v2): wrecs[(layer * 6 + wave) * RS]
        const uint32_t* wr = V2 ? wrecs + (size_t)wave_u * rec_stride_wave(DMAX) : recs; // builds without packed nodes read the per-layer records
        // (word 1 carries nothing: it is loaded with the header only for the first record, which keeps the scalar loads of the kernel as measured)
        uint32_t nhdr = wr[0], nw1 = wr[1];
        uint32_t nent[2 * DMAX];
#pragma unroll
        for (int k = 0; k < 2 * DMAX; k += PF) nent[k] = wr[4 + k]; // (PF = 2 DMAX: word 0 only, never used)
        DVBS2_WAIT_VM0(); // (the first layer's messages: once per sweep, so that inside the loop no path has a load pending at a layer boundary)
        // the same for the first layer's RECORD: with its scalar loads pending on the path into the loop the compiler waits for them at the
        // first use of the header -- behind the next record's prefetch, which every iteration then waits for as soon as it has issued it
        // (an empty asm statement that "uses" the loaded words: the compiler has to complete the loads in front of it; an explicit s_waitcnt
        // alone does not hold them -- loads of constant memory are moved across it). First measured on the plain class-8 build: B4 119.6 ->
        // 115.9 k without it; re-measured once B4 ran the packed one-frame build: B4 133.2 -> 134.5 k, 2/5 normal +0.7 %, 3/5 +1 %, others +-0.5 %.
        asm volatile("" : "+s"(nhdr), "+s"(nw1), "+s"(nent[0]));
        for (int i = 0; i < q; i++) {
            if constexpr (kRun) {
                // Run loop (see kRun): a maximal stretch of consecutive regular layers whose record of THIS wave is packed and has one degree.
                // The degree dispatch and the header decode happen once per run, and the trip is unrolled by two over ping-pong registers:
                // the record (A / B) and the messages (pre / pb) a trip has fetched ahead are what the next trip works on, where it lies.
                // What a trip keeps of the layer loop: the per-layer barrier bit, the message prefetch behind the barrier, the vmcnt(0) in
                // front of the stores. The next RECORD is fetched from inside the node, behind its input phase (the hook of check_node_v2,
                // RUN): scalar memory shares its counter with LDS, so at the trip's head the three record loads sat under the node's first
                // LDS wait, which then could not be counted over the six byte reads either (notes/r12_trip_waits.md).
                // What it does not hold (notes/r10_straight_trip.md): a frame's first sweep -- it loads no messages, and as
                // an arm of the trip it cost every trip a message copy and three flag registers; that sweep takes the packed arm of the
                // layer loop below --, a layer index (the message offset is the induction variable, the record to fetch ahead a running
                // pointer) and the table's last layer, behind which that pointer would have to wrap: a run ends in front of it. A run
                // ends at the first prefetched header that differs from the run's first one in degree, format or block. Waves of a frame
                // may cut their runs differently (bit 13 is per wave); the barrier bit is the layer's, so every wave meets the same
                // barriers on either path.
                if (work && !zero_msgs && i + 1 < q && (nhdr & kRecPacked) && (nhdr >> kRecBlockShift) >= (uint32_t)kM) {
                    auto run = [&](auto degc) {
                        constexpr int D = decltype(degc)::value;
                        // what a header must share with the run's first one to continue it: degree, format and block (equal blocks: both regular)
                        constexpr uint32_t kKeyMask = (~0u << kRecBlockShift) | kRecPacked | 0xffu;
                        const uint32_t key = nhdr & kKeyMask;
                        uint32_t ha = nhdr, hb, ea[2 * DMAX], eb[2 * DMAX], pb[MW];
                        // (readfirstlane: the words are uniform, and the instruction folds away where the layer loop holds them in scalar registers.
                        // It cuts the register-class link between the layer loop's copy of a record and the run loop's: with the record loads
                        // issued from inside the node the compiler keeps words 0-3 of BOTH copies in VGPRs without it -- four v_mov per pair of
                        // trips --; with it the layer loop alone does, and a run pays four lane reads at its entry. notes/r12_trip_waits.md)
#pragma unroll
                        for (int k = 0; k < 2 * DMAX; k++) ea[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)nent[k]);
                        const uint32_t* nrec = wr + (size_t)(i + 1) * RSW; // the record the next trip fetches ahead: a running pointer
                        int sa = i * kLayerBytes, sb;                       // scalar byte offset of a trip's messages
                        const int s_last = (q - 1) * kLayerBytes;           // the last layer's: never reached inside a run
                        const int rowb360 = row + lb + kM;                  // the base of a fix slot's lanes below the wrap point (check_node_v2, RUN)
                        // Parity carry (check_node_v2, RUN): the first trip's barrier is taken here, then its previous-parity byte is read into the
                        // carry (a one-wave walk layer in front of the run writes that byte from another wave: not before the barrier); behind the
                        // run's last trip the own-parity byte that trip kept back goes to LDS, so that every path outside the run finds LDS as ever.
                        // (Timing builds: this barrier lies in front of the first trip's TSTAMP(tA), so tm_bar and the per-layer sums leave out the barrier of a run's first layer.)
                        if ((ha & (1u << kRecSyncShift)) != 0u) { lds_barrier(); ha &= ~(1u << kRecSyncShift); }
                        uint32_t carry = (uint32_t)lds_rd(row + lb + (int)ea[D - 1]) << ((D & 1) ? 24 : 8);
                        auto flush_parity = [&](const uint32_t* E /*the record of the run's last trip*/) {
                            const int a = row + lb + (int)E[D - 2];
                            if constexpr ((D & 1) != 0) lds_wr_hi(a, carry >> 8); else lds_wr(a, (int)(carry >> 8));
                        };
// one trip: the layer of record (H, E) with the messages P at offset S; the next layer's record goes to (NH, NE), its messages to NP, its offset to NS
// (a row's messages are addressed as rowm + S: the per-lane part is loop invariant, so the trip has no scalar add per load and store)
#define DVBS2_RUN_TRIP(H, E, P, S, NH, NE, NP, NS) { \
                            TSTAMP(tA); \
                            NS = S + kLayerBytes; \
                            if (__builtin_expect((H & (1u << kRecSyncShift)) != 0u, 1)) lds_barrier(); \
                            TSTAMP(tB); tm_bar += tB - tA; \
                            uint32_t nm[MW]; \
                            msg_load(NP, NS, rowm); \
                            check_node_v2<D, DMAX, TC, true>(E, row + lb, P, nm, [&]() { \
                                asm volatile("" ::: "memory"); \
                                NH = nrec[0]; \
                                _Pragma("unroll") for (int k = 0; k < 2 * DMAX; k++) NE[k] = nrec[4 + k]; \
                                nrec += RSW; \
                                asm volatile("" ::: "memory"); \
                            }, rowb360, &carry); \
                            DVBS2_WAIT_VM0(); \
                            msg_store(nm, S, rowm); \
                            TSTAMP(tC); tm_body += tC - tB; \
                            if (TIMING && tdbg && f == 0 && tid == 0) tdbg[(size_t)n_frames * 48 + S / kLayerBytes] += tC - tA; }
                        // two tests, two branches that are not taken inside a run (the empty statement keeps them from being merged into flag arithmetic)
                        auto run_ends = [&](uint32_t h, int s) {
                            if (__builtin_expect((h & kKeyMask) != key, 0)) return true;
                            asm volatile("");
                            return (bool)__builtin_expect(s >= s_last, 0);
                        };
                        for (;;) {
                            DVBS2_RUN_TRIP(ha, ea, pre, sa, hb, eb, pb, sb)
                            if (run_ends(hb, sb)) { // the run ends behind an odd trip: what was fetched ahead moves to where the layer loop expects it
                                flush_parity(ea);
                                nhdr = hb;
#pragma unroll
                                for (int k = 0; k < 2 * DMAX; k++) nent[k] = eb[k];
#pragma unroll
                                for (int w = 0; w < MW; w++) pre[w] = pb[w];
                                i = sa / kLayerBytes;
                                break;
                            }
                            DVBS2_RUN_TRIP(hb, eb, pb, sb, ha, ea, pre, sa)
                            if (run_ends(ha, sa)) {
                                flush_parity(eb);
                                nhdr = ha;
#pragma unroll
                                for (int k = 0; k < 2 * DMAX; k++) nent[k] = ea[k];
                                i = sb / kLayerBytes;
                                break;
                            }
                        }
#undef DVBS2_RUN_TRIP
                    };
                    switch (nhdr & 0xffu) { DVBS2_DEGREES_3_7(DVBS2_RUN_CASE) DVBS2_RUN_CASE(8) default: break; }
                    continue;
                }
            }
            const uint32_t hdr = nhdr;
            uint32_t ent[2 * DMAX];
#pragma unroll
            for (int k = 0; k < 2 * DMAX; k++) ent[k] = (PF <= 2 * DMAX - 1 && k % PF == 0) ? nent[k] : wr[(size_t)i * RSW + 4 + k];
            const int inext = i + 1 < q ? i + 1 : 0; // the layer whose record and messages are fetched ahead
            const uint32_t* nrec = wr + (size_t)inext * RSW;
            auto prefetch = [&](uint32_t after) {
                const uint32_t* p = nrec; (void)after;
                nhdr = p[0];
                if constexpr (PF <= 2 * DMAX - 1) {
#pragma unroll
                    for (int k = 0; k < 2 * DMAX; k += PF) nent[k] = p[4 + k];
                }
            };
            // a packed-node layer (bit 13) may issue these loads from inside the node; the others here
            // Degree classes up to kPabMaxDmax issue them BEHIND the layer's barrier: in front of it the wave waits for them (lgkmcnt(0)
            // of the barrier and of the first use of the header) as soon as it has issued them. Measured: B4 +0.7 %, 1/3 normal +1.5 %,
            // S2X 9/20 +1.2 %, 1/4 normal +1.4 %; the classes 12-32 lose up to 5 % (S2X_TABLE_B16) -- class 8 only.
            constexpr int kPabMaxDmax = 8;
            constexpr bool kPab = DMAX <= kPabMaxDmax;
            if constexpr (!kPab) prefetch(0u);
            const int deg = (int)(hdr & 0xffu) + 2;
            const int nc = (int)((hdr >> 8) & 0xfu);
            lds_u32_t* htab = ((hdr >> 12) & 1u) ? sv : nullptr; // lane-chain scratch: the sign-vector area is idle during a sweep
            const int block = (int)(hdr >> 16);
            int block2 = 0; // hazard layers: rows per outer block of the two-level walk (0: off)
            if constexpr (HZ2 || (kTlc<DMAX, HZ2> && !SOFT && MINW == 1)) { if (block < kM) block2 = (int)wr[(size_t)i * RSW + 2]; }
            const bool layer0 = (i == 0);
            const int mso = i * kLayerBytes; // scalar byte offset of this layer's message records
            TSTAMP(tA);
            if (hdr & 0x8000u) lds_barrier();
            if constexpr (kPab) { asm volatile("" ::: "memory"); prefetch(0u); }
            TSTAMP(tB); tm_bar += tB - tA;
            if (block >= kM) {
                // regular layer: all 360 checks at once
                if (work) {
                    const int jj = row;
                    const bool v2 = V2 && ((hdr >> 13) & 1u);
                    // v2: this wave's record is in the packed node's format (two's complement messages)
                    uint32_t mw[MW], nm[MW];
                    take_msgs(mw, pre, zero_msgs, v2 ? 0u : 0x80808080u, inext * kLayerBytes, rowm);
                    // (kRun: a packed record of a working wave gets here in a frame's first sweep and at the table's last layer only -- the run loop took the others)
                    if constexpr (V2) { if (v2) { DVBS2_V2_SWITCH } else DVBS2_DEG_SWITCH } else DVBS2_DEG_SWITCH
                    DVBS2_WAIT_VM0();
                    msg_store(nm, mso, rowm);
                }
                TSTAMP(tC); tm_body += tC - tB;
                if (TIMING && tdbg && f == 0 && tid == 0) tdbg[(size_t)n_frames * 48 + i] += tC - tA; // per-layer cycles of frame 0, wave 0 (incl. its barrier)
            } else {
                if (nc != kHazardWalk) {
                    // sequential-order hazard inside the layer: check_node_hazard (every thread takes every barrier)
                    const int jj = row;
                    // hv2: packed single-pair chain (check_node_chain_v2): two's complement messages
                    const bool hv2 = V2 && ((hdr >> 13) & 1u);
                    uint32_t mw[MW], nm[MW];
#pragma unroll
                    for (int w = 0; w < MW; w++) mw[w] = (work && !zero_msgs) ? pre[w] : (hv2 ? 0u : 0x80808080u);
                    if (work && i + 1 < q && !zero_msgs) msg_load(pre, mso + kLayerBytes, rowm);
                    // hvp: the generic hazard node with the packed first / last phase (header bit 14 of this wave's record; every wave of the
                    // layer runs the same ordered phase, whichever form its own record has)
                    const bool hvp = V2 && v2p_class(DMAX) && ((hdr >> 14) & 1u);
                    if constexpr (V2 && DMAX <= 16) { // (the chain node's register state costs the high-degree builds more than it saves: not built there)
                        if (hv2) {
                            lds_u32_t* htab16 = lds_align16<lds_u32_t>(sv); // 16-byte records
                            DVBS2_CHAIN_SWITCH
                        } else DVBS2_HAZ_SWITCH
                    } else if constexpr (V2 && v2p_class(DMAX)) { if (hvp) { DVBS2_HAZP_SWITCH } else DVBS2_HAZ_SWITCH }
                    else DVBS2_HAZ_SWITCH
                    DVBS2_WAIT_VM0(); // (on every path, so that nothing is pending behind it whatever the branch)
                    if (work) msg_store(nm, mso, rowm);
                } else {
                    // too many hazard entries: the first wave of the half walks the 360 checks alone in ascending
                    // chunks of min(B_i, 64) (LDS operations of one wave execute in order: no barrier between chunks)
                    if (!finished && wave == 0) {
                        const int chunk = block < 64 ? block : 64;
                        for (int start = 0; start < kM; start += chunk) {
                            const int jj = start + lane;
                            if (lane < chunk && jj < kM) {
                                uint32_t mw[MW], nm[MW];
#pragma unroll
                                for (int w = 0; w < MW; w++) mw[w] = zero_msgs ? 0x80808080u : MSG_LD(mso, w, jj * kMsgRowBytes);
                                DVBS2_DEG_SWITCH
#pragma unroll
                                for (int w = 0; w < MW; w++) MSG_ST(nm[w], mso, w, jj * kMsgRowBytes);
                            }
                        }
                    }
                    lds_barrier();
                    if (work && i + 1 < q && !zero_msgs) msg_load(pre, mso + kLayerBytes, rowm);
                    DVBS2_WAIT_VM0(); // (rare path; keeps "nothing pending at the end of a layer" true on EVERY path, see DVBS2_WAIT_VM0)
                }
                TSTAMP(tC); tm_conf += tC - tB;
                if (TIMING && tdbg && f == 0 && tid == 0) tdbg[(size_t)n_frames * 48 + i] += tC - tA;
            }
        }
        TSTAMP(tA);
        lds_barrier();
        TSTAMP(tB); tm_bar += tB - tA; tm_sweep += tB - tS1;
        if (!finished) it++;
    }
    if (TIMING && tdbg && lane == 0 && have_frame) {
        unsigned long long* o = tdbg + ((size_t)f * 6 + wave) * 8;
        o[0] = tm_load; o[1] = tm_synd; o[2] = tm_sweep; o[3] = tm_bar; o[4] = tm_body; o[5] = tm_conf; o[6] = (unsigned long long)it; o[7] = tm_s1;
    }

    if (have_frame && !untouched) {
        if (tid == 0) { iters[f] = it; good[f] = is_good ? 1 : 0; }
        uint2* dst = reinterpret_cast<uint2*>(state + (size_t)f * N);
        for (int c = tid; c < N / 8; c += kHalf) { const v2u32 v = *reinterpret_cast<const lds_v2u_t*>(lds + 8 * c); dst[c] = make_uint2(v.x ^ kObState, v.y ^ kObState); }
    }
    if constexpr (SOLO) { // give the CU's pattern slot back
        if (tid == 0) __hip_atomic_fetch_add(cu_slots + solo_slot, solo_pat ? -0x10000 : -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace dvbs2
