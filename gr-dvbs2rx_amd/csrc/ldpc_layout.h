// ldpc_layout.h -- what the host planner (ldpc_plan.cpp) and the sweep kernels (ldpc_kernel.hpp, ldpc_kernel_pr.hpp) must agree on:
// the record format, the LDS sizes, the limits of the hazard paths and the list of builds. No HIP: plain constexpr, usable from
// device code under hipcc and from a host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dvbs2 {

constexpr int kM = 360;
constexpr int kMsgStride = 384;     // message slots per (layer, word)
// Message records of the classic sweep kernel, per frame: [layer][word][384 rows] dwords -- a wave's access to one word is contiguous --,
// except with TWO words per check (the degree class 8): [layer][384 rows][2 words], one 8-byte record per row, loaded and stored with one
// dwordx2 access. Word w of row r of a layer lies at byte  r * msg_row_bytes(mw) + w * msg_word_step(mw)  behind the layer's offset
// (layer * mw * kMsgStride * 4 in both forms: the allocation is the same).
constexpr int msg_row_bytes(int mw) { return mw == 2 ? 8 : 4; }
constexpr int msg_word_step(int mw) { return mw == 2 ? 4 : kMsgStride * 4; }
constexpr int kSvWords = 14;        // sign-vector dwords per 360-bit group (360 bits + 32-bit wrap extension, even for b64 stores)

// Layer record (uniform data, read with scalar loads): RS = 2*DMAX + 4 dwords.
//   word 0: cnt | sync_before << 15 | block << 16
//   words 4+2k, 5+2k (k < deg): entry k as  S0 = 360*g + rot  and  thr = 360 - rot
// Entry k addresses the LDS window [360*g, 360*g + 360) rotated by rot: check row j touches byte
// 360*g + (j + rot) mod 360 = (j < thr ? S0 + j : S0 + j - 360).
constexpr int rec_stride(int dmax) { return 2 * dmax + 4; }       // per-layer records (recs)
constexpr int rec_stride_wave(int dmax) { return 2 * dmax + 12; } // per-(layer, wave) records of the packed builds (wrecs)
// word 0 of a record, all fields (bits 0-7: cnt)
constexpr int kRecNcShift = 8;                   // bits 8-11: entries of the ordered phase of a hazard layer (2, 4, 8, 12; kHazardWalk)
constexpr uint32_t kRecChain = 1u << 12;         // the hazard pair (entries 0, 1, host-oriented) is walked as a lane chain
constexpr uint32_t kRecPacked = 1u << 13;        // (layer, wave) record in the packed format (check_node_v2 and its kin)
constexpr uint32_t kRecPackedHazard = 1u << 14;  // ... of a hazard layer with the packed first / last phase (V2P)
constexpr int kRecSyncShift = 15;                // bit 15: sync_before
constexpr int kRecBlockShift = 16;               // bits 16+: block
// the kernels' stop_on_good argument: bit 0 = stop at the first good syndrome test, then
constexpr int kFlagSoftBarrier = 2; // frame barriers in software (the soft builds)
constexpr int kFlagGroupSync = 4;   // group-synchronous stop (group_decide)
constexpr int kFlagPrSharedSv = 8;  // parity in records: one sign-vector area per workgroup, the frames take turns
// In FRONT of the per-layer records (recs[-kRecHeaderWords ..]): what the group-synchronous stop needs (group_decide) -- the base of the
// handle's `iters` array (the kernel's own `iters` argument minus it = the first frame of this launch), the base of the per-group words
// and the group size. Kept out of the kernel's argument list on purpose: arguments stay live in SGPRs for the whole kernel, and the
// one-frame builds of the degree class 16 answered three more of them with 25 more spilled scalars and 2-3 % (measured); here they are
// fetched with two scalar loads once per update, by the lane that reports.
constexpr int kRecHeaderWords = 8; // [0,1] iters base, [2,3] base of the per-frame status words (group_decide), [4] group size, [5] polls before a waiting member gives up, rest unused
constexpr int kGroupSpinMax = 1 << 12; // polls of ~2 us
// per frame: N LLR bytes, then the sign-vector area (syndrome test; scratch of the ordered hazard phases during a sweep:
// at least kChainScratchWords dwords, which is what short frames get instead of their small sign-vector area), then 8 flag words
// largest block walked as a register chain -- round 4: 128 -> 180 (blocks 129..180 are three-step block-scheme layers otherwise): 3/4 normal
// +1.6 %, 3/5 +1.3 %, B4 / 2/5 normal +0.4 %
constexpr int kChainMaxBlock = 180;
constexpr int kChainScratchWords = (kM + kChainMaxBlock) * 5 + 4;               // (360 + block) x (16-byte record + 4-byte log) + 16 bytes: the records are 16-byte aligned and the area starts at N, which is 8 mod 16 for short frames
constexpr int sv_area_words(int N) { return (N / kM) * kSvWords > kChainScratchWords ? (N / kM) * kSvWords : kChainScratchWords; }
constexpr size_t half_lds_bytes(int N) { return ((size_t)N + (size_t)sv_area_words(N) * 4 + 32 + 15) / 16 * 16; }
// parity in records (ldpc_kernel_pr.hpp): K information LLRs + parity row q-1 per frame
constexpr size_t pr_half_bytes(int K) { return ((size_t)K + kM + 15) / 16 * 16; }
// two frames + sign-vector areas: one PER FRAME (round 5: the frames run their full syndrome tests at the same time), or ONE shared by the
// workgroup where two do not fit twice into the 160 KB of a CU (normal frames forced onto this kernel: the frames then take turns; bit 3 of the flag word)
constexpr size_t pr_lds_bytes(int N, int K, bool shared_sv = false) { return 2 * pr_half_bytes(K) + (shared_sv ? 1 : 2) * (size_t)(N / kM) * kSvWords * 4 + 64; }

// two-level lane chain (check_node_hazard): the degree class 32 without the heavy-hazard paths (9/10 normal); not in the builds with software
// frame barriers, which only tables without hazard layers run (S2X 154/180 lost 2.5 % to the larger kernel)
// Which degree classes carry it is MEASURED (MI355X, interleaved A/B of whole tables, notes/r03_experiments.md): at run time the chain is
// never slower than the ordered steps it replaces (9/10 normal + 13 %, 3/5 normal + 10 %, short 5/6 + 4 %, 3/4 normal + 2.4 %), but
// compiling it in costs the packed / one-frame builds of the classes 12 and 28 eight percent on every table (2/3, T2 2/3, 8/9 normal)
// and the class 20 what its one table gains -- so: 16 (3/4 normal + 5 % net, short 5/6 + 2 %, short 2/3 - 4 %), 24 (5/6 normal + 1.3 %),
// 32 (9/10 normal + 8 %).
constexpr bool tlc_class(int dmax) { return dmax == 16 || dmax == 24 || dmax == 32; }
// Hazard layers with the packed first / last phase (check_node_hazard<..., V2P>, round 5): compiled into the packed builds of the degree
// classes from 20 up -- the classes whose hazard layers all took the plain node (no packed chain node there).
constexpr bool v2p_class(int dmax) { return dmax >= 20; }
// "pure" packed builds (kPure in ldpc_layered_kernel) -- measured (round 5, interleaved A/B): class 32 (9/10 normal) 80.2 -> 83.9 k;
// 28 (8/9) 95.9 -> 91.2 k, 24 (5/6) 76.9 -> 74.2 k
constexpr bool v2_pure_class(int dmax) { return dmax >= 32; }
// fix slots per record: masks live in record words 4 + dmax + 2 k. The degree class 32 has ten: with them every wave record of S2X 154/180
// fits the packed format (with 8 two of its 150 did not).
constexpr int v2_nfix(int dmax) { return dmax == 32 ? 10 : dmax / 4; }

// LDS scratch of a lane chain with block size B: (360 + B) per-row records (dwords) + as many log bytes
constexpr int lane_chain_words(int block) { return (kM + block) + (kM + block + 3) / 4; }
constexpr int kLaneChainMaxDeg = 28;                                  // not instantiated for the big variants nor for the
                                                                      // 80-VGPR parity-in-records kernel (registers); hazard nodes with
                                                                      // the packed first / last phase (their state is smaller) have it at
                                                                      // every degree: 9/10 normal 83.9 -> 86.3 k (round 5)
constexpr int kMaxHazard = 8;     // ordered entries per check in the common builds, kMaxHazardHz2 in the HZ2 builds (ldpc_layered_kernel)
constexpr int kMaxHazardHz2 = 12;
constexpr int kMaxHazard12Dmax = 28; // (the degree class 32 has the two-level walk only: twelve ordered entries on top of 30 edges do not fit its registers)
constexpr int kHazardWalk = 15; // header code: too many hazard entries, fall back to the single-wave chunk walk

constexpr int kCuSlots = 16 * 8 * 2 * 16; // per-CU pattern counters of the one-frame builds, indexed by hw_cu_index() (ldpc_kernel.hpp)

// The build of the sweep kernel a handle runs, decided once per table by the host (ldpc_plan.cpp). The classic kernel's builds exist
// in the degree classes the k*Built rules of ldpc_launch.h and ldpc_inst.hpp give; the parity-in-records builds (ldpc_kernel_pr.hpp) in the class 8 only.
enum class LdpcBuild : uint8_t {
    plain,       // pair workgroups, scalar nodes
    packed,      // pair workgroups with the packed nodes (check_node_v2, check_node_chain_v2)
    solo,        // one frame per workgroup (kSoloBuilt)
    packed_solo,
    hz2,         // the heavy-hazard paths (kHz2Built)
    soft,        // software frame barriers (kSoftBuilt)
    packed_soft,
    dense,       // 80 VGPRs, two workgroups per CU (kDenseBuilt)
    pr,          // parity in records: two-dword records, plain nodes
    pr_w1,       //                    one-dword records (check degree <= 4)
    pr_packed,   //                    two-dword records, packed nodes in the regular middle layers
};
constexpr int kLdpcBuilds = (int)LdpcBuild::pr_packed + 1;
constexpr bool is_solo(LdpcBuild b) { return b == LdpcBuild::solo || b == LdpcBuild::packed_solo; }
constexpr int kSoloMaxDmax = 16; // one-frame workgroups (128 VGPRs) up to this degree class (round 6 bound, notes/r06_experiments.md)

} // namespace dvbs2
