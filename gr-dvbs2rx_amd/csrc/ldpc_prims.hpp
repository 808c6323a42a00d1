// ldpc_prims.hpp -- what every LDPC check node and both sweep kernels (ldpc_kernel.hpp, ldpc_kernel_pr.hpp) are built from: the thread
// mapping, LDS pointer types and accessors, the frame barriers, the group-synchronous stop, the pinned-instruction helpers and the one list
// of check degrees. The record format and the constants shared with the host planner: ldpc_layout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ldpc_layout.h"

// s_waitcnt vmcnt(0) (expcnt, lgkmcnt untouched) that memory operations are not moved across, in front of the stores of a layer's new
// messages. The compiler waits for the NEXT layer's prefetched messages (loaded at the head of this layer) with vmcnt(0) -- loads and
// stores share the counter and across this loop's control flow it cannot count them -- and, left alone, places that wait at their first
// use, i.e. right AFTER the stores it has just issued: every wave of the workgroup then sat through the L2's acknowledgement of its stores
// at every layer boundary. Waiting first costs nothing (the prefetch is a layer old) and leaves the stores a whole layer to complete; no
// register is added. Measured (interleaved A/B): 1/4 normal +7 %, B4 +3.6 %, 1/3 normal +8 %, 3/4 normal +3 % (23 tables, none loses).
// (kWaitStore in scope: not in the builds with software frame barriers -- S2X 154/180 lost 4 % with it)
#define DVBS2_WAIT_VM0() do { if (kWaitStore) { asm volatile("" ::: "memory"); __builtin_amdgcn_s_waitcnt(0x0f70); asm volatile("" ::: "memory"); } } while (0)

// The check degrees, named once: every degree dispatch (ldpc_kernel.hpp, ldpc_kernel_pr.hpp) is `switch (deg) { LIST(ITS_CASE) default: ... }`
// with a case macro of its own. The list is cut where the dispatches begin and end: the plain and packed nodes start at degree 3, the hazard
// nodes (two ordered entries + two parity entries) at 4, and the parity-in-records kernel stops at 7.
#define DVBS2_DEGREES_4_7(X) X(4) X(5) X(6) X(7)
#define DVBS2_DEGREES_8_32(X) X(8) \
        X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) \
        X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
#define DVBS2_DEGREES_3_7(X) X(3) DVBS2_DEGREES_4_7(X)
#define DVBS2_DEGREES_4_32(X) DVBS2_DEGREES_4_7(X) DVBS2_DEGREES_8_32(X)
#define DVBS2_DEGREES_3_32(X) X(3) DVBS2_DEGREES_4_32(X)

namespace dvbs2 {

// Thread mapping: a workgroup of 12 wavefronts decodes a PAIR of FECFRAMEs in lockstep; wavefronts 0-5 own
// frame 2b, wavefronts 6-11 own frame 2b+1. Inside a half, thread t (< 360) owns check row t of every
// circulant layer. Two frames are what the 160 KB of LDS hold (2 x (64800 + 9360) bytes for normal frames);
// putting them in ONE workgroup makes the hardware spread its 12 waves 3 per SIMD, all in the same phase of
// the same layer, so the per-layer barrier costs no load-imbalance wait (two independent 6-wave workgroups
// land 2,2,1,1 on the SIMDs and spend a quarter of their time waiting for the doubly loaded ones).
constexpr int kHalf = 384;          // threads per frame (6 wavefronts; threads 0..359 active)
constexpr int kThreads = 2 * kHalf; // 12 wavefronts

// EVERY access to LDS goes through a pointer whose TYPE says address space 3. A generic pointer that the compiler cannot trace back
// to the shared array (a function parameter, a pointer rebuilt from an integer for alignment, any `volatile` access) becomes a FLAT
// instruction: 64-bit address arithmetic, the long way round through the vector-memory path, and -- because flat loads return out of
// order with buffer loads -- an `s_waitcnt vmcnt(0) lgkmcnt(0)` at every use, which also waits for the message prefetch from HBM
// and serialises "rows in flight". Round 4 found the lane-chain walks, their operand tables and logs, the flag words and the
// software frame barrier all compiled that way (1 400 flat instructions in the degree class 8 alone): ~140 cycles per chain row.
typedef __attribute__((address_space(3))) uint8_t lds_byte_t;
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) int lds_i32_t;
typedef __attribute__((address_space(3))) float lds_f32_t;
typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef uint32_t v2u32 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) v4f32 lds_v4f_t;
typedef __attribute__((address_space(3))) v2u32 lds_v2u_t;
template <class T> __device__ __forceinline__ T* lds_align16(lds_u32_t* p) { return reinterpret_cast<T*>(((uint32_t)(size_t)p + 15u) & ~15u); }
__device__ __forceinline__ int wrap360(int t) { return t >= kM ? t - kM : t; }

// Barrier of ONE FRAME's six waves. The two frames of a workgroup share a CU only to get three waves on every SIMD
// (2+1 / 1+2: two separate 6-wave workgroups land 4,2,3,3 -- tools/ubench/placement.hip); nothing else couples them.
// With the hardware barrier both frames stall whenever either one is waiting for its slowest wave, for an LDS round trip
// or for an ordered hazard step; a barrier per frame lets the other frame's waves take the idle issue slots. gfx950 has
// no named barriers, so it is a counter in the frame's LDS region: every wave adds one (LDS executes a wave's operations
// in order, so its earlier writes are in place when the add lands) and polls until the count reaches the expected multiple of 6.
__device__ __forceinline__ void frame_barrier(volatile lds_i32_t* ctr, int& epoch, int lane)
{
    // (Round 4, with no FLAT access left in the kernel: the barrier without the wait for outstanding vector memory operations that
    // __syncthreads() implies -- s_waitcnt lgkmcnt(0) + s_barrier -- measured again: +-0.3 % on every BASELINE table. Not used.)
    if (!ctr) { __syncthreads(); return; } // hardware barrier of the workgroup (the default)
    epoch += 6;
    asm volatile("" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(const_cast<lds_i32_t*>(ctr), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (*ctr - epoch < 0) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}
#define lds_barrier() frame_barrier(hb_ctr, hb_epoch, hb_lane)
// The same where only LDS (the flag words) is handed over: without the wait for outstanding vector memory operations that
// __syncthreads() implies -- the group report of group_decide() is two fire-and-forget atomics whose acknowledgement would
// otherwise be waited for at the next barrier (short frames: 1.4 % of a sweep, measured).
__device__ __forceinline__ void frame_barrier_lds(volatile lds_i32_t* ctr, int& epoch, int lane)
{
    if (ctr) { frame_barrier(ctr, epoch, lane); return; }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
#define lds_only_barrier() frame_barrier_lds(hb_ctr, hb_epoch, hb_lane)

// Group-synchronous stopping rule. The reference decodes a SIMD batch of G frames in lockstep and stops the whole batch at the
// first update count at which EVERY lane passes the syndrome test (while (bad(any lane) && --trials >= 0),
// layered_decoder.hh:153). Frames of one group are dispatched together (consecutive workgroups) and run the same instruction
// stream, so they can simply agree after every test. Round 5: ONE STATUS WORD PER FRAME in global memory, written only by that frame,
//   status[f] = (update count of the test + 1) << 1 | passed          (0 = nothing reported yet; zeroed per call)
// A member reports with ONE relaxed store (fire and forget). A member that FAILS at count `it` knows the group goes on and does not
// wait. A member that PASSES reads the words of all members of its group (the first wave of the frame: lane m reads member m, one
// 256-byte access) and decides on them alone:
//   some member is PAST `it` (it only advances past a count at which a failure is known) or failed AT `it`   -> one more update (0)
//   every member passed AT `it`                                                                              -> stop (1)
//   else some member has not reported for `it` yet                                                           -> poll again
// Every member therefore leaves at the first count at which all pass -- the reference's count -- and no resume pass is needed.
// Each word has a single writer and its value only grows, so the decision needs no ordering BETWEEN words and no read-modify-write:
// rounds 3-4 kept {arrive, lastbad} per group, updated by a failing member with two separate relaxed atomics whose order at the L2
// the memory model does not promise; that dependence is gone. Relaxed at agent scope as before (a release /
// acquire at agent scope writes back and invalidates the per-XCD L2: 12 % of the never-converging batch, measured in round 3).
// Returns 2 = gave up waiting after spin_max polls (members not co-resident for milliseconds: never observed; the frame then stops
// at its own good point like in rounds 1-2 and the host-side resolution, ldpc_group_targets_kernel + resume launches, finishes the
// group -- a frame only ever advances past a count at which some member is known to have failed, so it can never overshoot).
// Called by ALL lanes of the frame's first wave (wave-uniform arguments); groups of at most 64 frames.
__device__ __forceinline__ int group_decide(int* st /*status words of this frame's group*/, int members, int me /*this frame's index in its group*/,
                                            int it, bool good, int lane, int spin_max = kGroupSpinMax)
{
    const int mine = ((it + 1) << 1) | (good ? 1 : 0);
    // (measured against an atomic max without a returned value -- the same thing for a value that only grows --: identical rates on
    // short 1/4, 2/5, 1/4 normal, B4 and medium 1/5, where a frame reports every 40-90 us: notes/r05_experiments.md)
    if (lane == 0) __hip_atomic_store(st + me, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!good) return 0; // (nothing is waited for)
    for (int spin = 0;; spin++) {
        int s = mine; // lanes without a member, and this frame itself (its own store need not be visible to its own load yet), are neutral
        if (lane < members && lane != me) s = __hip_atomic_load(st + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool goes_on = s > mine || s == mine - 1; // a later count, or this count failed
        const bool missing = s < mine - 1;              // an earlier count (or nothing yet)
        if (__ballot(goes_on) != 0) return 0;
        if (__ballot(missing) == 0) return 1;
        if (spin >= spin_max) return 2;
        __builtin_amdgcn_s_sleep(8);
    }
}

// Pinned instruction selection for the two spots where the compiler's canonical form costs more issue slots.
// clamp(a + b + 128, 0, 255) as v_add3_u32 + v_med3_i32 (the compiler emits add, max, add, min).
__device__ __forceinline__ int sat_sum_u8(int a, int b)
{
    int r; // one asm statement: between two the compiler puts an s_nop (it cannot see that the pair has no hazard)
    asm("v_add3_u32 %0, %1, %2, %3\n\tv_med3_i32 %0, %0, 0, %4" : "=&v"(r) : "v"(a), "v"(b), "s"(128), "s"(255));
    return r;
}
// R2: mag = clamp(|Lb - mb| - 1, 0, 126) as v_sad_u16 + v_med3_i32 (the compiler splits the clamp into max + min)
__device__ __forceinline__ int mag_offset(int Lb, int mb)
{
    int r;
    const int a = (int)__builtin_amdgcn_sad_u16((uint32_t)Lb, (uint32_t)mb, 0xffffffffu);
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(a), "s"(126));
    return r;
}
// LLR bytes are addressed with ABSOLUTE LDS addresses (the row index carries the frame's offset and the address of
// the dynamic LDS array): going through the array symbol costs one `v_add_u32 v, <lds_all>, v` per access, because the
// array's address is a link-time constant the compiler cannot fold into an address that inline asm produced.
__device__ __forceinline__ int lds_rd(int a) { return *reinterpret_cast<const lds_byte_t*>((size_t)(uint32_t)a); }
__device__ __forceinline__ void lds_wr(int a, int v) { *reinterpret_cast<lds_byte_t*>((size_t)(uint32_t)a) = (uint8_t)v; }
// the byte OFF behind a, through the typed pointer: the constant goes into the instruction's offset field (ds_read_u8 ... offset:OFF), no add
template <int OFF> __device__ __forceinline__ int lds_rd_at(int a) { return *(reinterpret_cast<const lds_byte_t*>((size_t)(uint32_t)a) + OFF); }
// Round 5: the builds with packed nodes keep the LLR bytes in LDS as TWO'S COMPLEMENT (TC): the packed arithmetic works on value << 8 in signed
// 16-bit halves, and with offset-binary bytes every pair paid one xor after its reads and one before its writes (8 of the ~110 VALU instructions
// of a degree-7 check). The scalar paths of such a build (layer 0, the ordered phase of hazard layers, waves whose record does not fit the
// packed format) convert at their LDS accesses; messages, the state in HBM and every other build stay as they were.
// Measured (interleaved A/B, all packed builds with and without): the degree class 8 gains (B4 135.4 -> 137.7 k, S2X 9/20 +0.7 %), every other
// class loses 0.2-3 % (3/4 normal -2.7 %, 4/5 -3 %, short 3/4 -2.9 %: their scalar paths pay the conversion, and removing 7 % of the packed
// node's VALU instructions buys almost nothing where the layer is as much bound by its message traffic and barriers) -- so: class 8 only.
constexpr int kTcMaxDmax = 8;
template <bool TC> __device__ __forceinline__ int lds_rdx(int a) { const int v = lds_rd(a); return TC ? (v ^ 0x80) : v; }          // offset-binary value of the LLR byte at a
template <bool TC> __device__ __forceinline__ void lds_wrx(int a, int v) { lds_wr(a, TC ? (v ^ 0x80) : v); }                        // store an offset-binary value
template <bool TC> constexpr uint32_t kObPair = TC ? 0u : 0x80008000u; // offset binary -> two's complement << 8 of a pair register
__device__ __forceinline__ int lds_address_of(const uint8_t* p) { return (int)(uint32_t)(size_t)(const lds_byte_t*)p; }

// LDS address of check row jj for entry (S0 = 360*g + rot, thr = 360 - rot): S0 + jj, minus 360 when jj >= thr.
// The canonical compare + select + add3 is three half-rate VALU instructions; this is four full-rate ones (2.5 vs 4.3
// cycles each on gfx950): subtract, sign mask, bitfield select between jj and jj - 360 (v_bitop3), add.
__device__ __forceinline__ int wrap_addr(int jj, int jjb, int jjb360, uint32_t S0, uint32_t thr)
{
    // jjb = jj + byte offset of this frame's LDS region (folded in here: no separate base add per access)
    int r;
    asm("v_subrev_u32 %0, %4, %1\n\t"
        "v_ashrrev_i32 %0, 31, %0\n\t"
        "v_bitop3_b32 %0, %0, %2, %3 bitop3:0xca\n\t"
        "v_add_u32 %0, %5, %0"
        : "=&v"(r) : "v"(jj), "v"(jjb), "v"(jjb360), "s"(thr), "s"(S0));
    return r;
}

// R3: the two smallest of N magnitudes. The kernel is bound by the VALU pipe and min/max/med3 are half-rate
// there, so the count matters: triples go through v_min3 + v_med3 (smallest and second smallest of three in two
// instructions), two sorted pairs merge in three, a single value folds in with two -- 9 instructions for seven
// values where the running (min0, min1) update needs 14.
__device__ __forceinline__ int vmin3_i32(int a, int b, int c) { int r; asm("v_min3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ int vmed3_i32(int a, int b, int c) { int r; asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
template <int N>
__device__ __forceinline__ void two_smallest(const int* v, int& m0, int& m1)
{
    static_assert(N >= 1, "empty set");
    int k;
    if constexpr (N == 1) { m0 = v[0]; m1 = 127; k = 1; }
    else if constexpr (N == 2) { m0 = min(v[0], v[1]); m1 = max(v[0], v[1]); k = 2; }
    else { m0 = vmin3_i32(v[0], v[1], v[2]); m1 = vmed3_i32(v[0], v[1], v[2]); k = 3; }
#pragma unroll
    for (; k + 3 <= N; k += 3) {
        const int g0 = vmin3_i32(v[k], v[k + 1], v[k + 2]), g1 = vmed3_i32(v[k], v[k + 1], v[k + 2]);
        const int t = max(m0, g0);
        m0 = min(m0, g0);
        m1 = vmin3_i32(t, m1, g1);
    }
#pragma unroll
    for (; k < N; k++) { m1 = vmed3_i32(m0, m1, v[k]); m0 = min(m0, v[k]); }
}

// R2 without its clamp: |Lb - mb| - 1 in [-1, 254]. Clamping to [0, 126] is monotone, so the two smallest clamped
// magnitudes are the clamps of the two smallest raw ones (two v_med3 per check instead of one per edge), and the
// selection "mag == min0 ? min1 : min0" becomes min0 + min1 - med3(raw, min0, min1): clamping raw into
// [min0, min1] gives min0 exactly when the clamped magnitude is the smallest one.
__device__ __forceinline__ int mag_raw(int Lb, int mb) { return (int)__builtin_amdgcn_sad_u16((uint32_t)Lb, (uint32_t)mb, 0xffffffffu); }
__device__ __forceinline__ int clamp_mag(int x) { int r; asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(126)); return r; }
constexpr int kMagAbsent = 0x7fff; // a link that does not exist (check (0,0)): above every raw magnitude

// low bytes of four 32-bit values -> one dword (two v_perm_b32 + or)
__device__ __forceinline__ uint32_t pack4_lo8(int a, int b, int c, int d)
{
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x0c0c0400u); // a.b0 | b.b0 << 8
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)d, (uint32_t)c, 0x04000c0cu); // c.b0 << 16 | d.b0 << 24
    return lo | hi;
}

__device__ __forceinline__ int pm_pack(int magp, int d) { return (int)__builtin_amdgcn_perm((uint32_t)magp, (uint32_t)d, 0x0c0c0400u); } // d.b0 | magp.b0 << 8
__device__ __forceinline__ int pm_inp(int pm) { return __builtin_amdgcn_sbfe(pm, 0, 8); }
__device__ __forceinline__ int pm_min_clamped(int p) { return clamp_mag((int)((uint32_t)p >> 8) - 1); } // R2 on a minimum: clamp(|x| - 1, 0, 126)

// + 360 on the lanes of `mask` (EXEC is saved and restored: the statement is valid under any execution mask)
__device__ __forceinline__ int fix_wrap(int ad, uint32_t mlo, uint32_t mhi)
{
    // (readfirstlane: a no-op for a value that already sits in an SGPR, and it keeps an SGPR that the register allocator
    // spilled to a VGPR lane from being handed to the scalar instruction as a VGPR)
    const unsigned long long mask = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)mhi) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)mlo);
    unsigned long long save;
    asm volatile("s_mov_b64 %1, exec\n\ts_and_b64 exec, exec, %2\n\tv_add_u32 %0, 0x168, %0\n\ts_mov_b64 exec, %1"
                 : "+v"(ad), "=&s"(save) : "s"(mask) : "scc");
    return ad;
}
// The same as a choice of the BASE the window offset is added to: b360 (= b + 360) on the lanes of `mask`, b on the others. One
// v_cndmask_b32 on the mask in its scalar register pair; EXEC is not touched and nothing here is an asm statement.
// (The mask words are record words of the run loop, uniform to the compiler, and are handed over as they are: a readfirstlane on them is a
// use that wants a VGPR, and with the record loads issued from inside the node that use made the compiler keep the whole record set of
// the run loop AND of the layer loop in VGPRs -- 8 v_mov per pair of trips, 16 bytes of scratch: notes/r12_trip_waits.md.)
__device__ __forceinline__ int wrap_base(int b, int b360, uint32_t mlo, uint32_t mhi)
{
    const unsigned long long mask = ((unsigned long long)mhi << 32) | mlo;
    return __builtin_amdgcn_inverse_ballot_w64(mask) ? b360 : b;
}

} // namespace dvbs2
