// ldpc_hip.hip -- layered offset-min-sum int8 LDPC belief propagation for DVB-S2/S2X/T2 on gfx950.
//
// What it computes (bit-exact contract): LDPCDecoder<SIMD<int8_t,W>, OffsetMinSumAlgorithm<...,
// NormalUpdate, FACTOR 2>>::operator() of the reference (lib/ldpc_decoder/layered_decoder.hh:143-160,
// lib/ldpc_decoder/algorithms.hh:151-207) for every frame, with the batch-coupled stopping rule of a
// G-frame SIMD batch, followed by the hard decision + MSB-first packing of
// ldpc_decoder_bb_impl::general_work (lib/ldpc_decoder_bb_impl.cc:432-442).
//
// Mapping (MI355X-first, not a translation of the lane-per-frame SIMD decoder):
//   * one FECFRAME per workgroup of 6 wavefronts; thread j (< 360) owns check node (layer i, lane j)
//     of every layer, i.e. one row of each circulant;
//   * the frame's N LLRs live in LDS for the whole decode (offset-binary bytes, parity part permuted
//     to [layer][lane]); a table entry (group g, shift s) is a rotated contiguous 360-byte window of it;
//   * the check-to-bit messages are private to the owning thread: they stream through L2/Infinity
//     Cache as coalesced dwords (4 int8 messages per dword), never through LDS;
//   * layers with two entries of the same group (sequential-order hazard of the reference's strictly
//     ordered update) are processed in ascending lane blocks of B_i (ldpc_schedule.h).
#include "ldpc_hip.h"
#include "ldpc_kernel.hpp"
#include "ldpc_kernel_pr.hpp"
#include "device_guard.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <optional>
#include <vector>

namespace dvbs2 {

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err_ = std::string(#x) + ": " + hipGetErrorString(e_); return; } } while (0)
#define HIP_RET(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { call_err_ = std::string(#x) + ": " + hipGetErrorString(e_); return -1; } } while (0)

// Per-group stopping rule of one reference SIMD batch: while (bad(any lane) && --trials >= 0) update(all lanes)
// (layered_decoder.hh:153). After a pass, every frame f sits at iters[f] updates with good[f] known there.
__global__ void ldpc_group_targets_kernel(const int* iters, const int* good, int* target, int* flag,
                                          int* ret, int n_groups, int G, int n_frames, int cap)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const int f0 = g * G, f1 = min(f0 + G, n_frames);
    int T = 0;
    for (int f = f0; f < f1; f++) T = max(T, iters[f]);
    bool aligned = true, all_good = true;
    for (int f = f0; f < f1; f++) {
        if (iters[f] != T) aligned = false;
        else if (!good[f]) all_good = false;
    }
    int tgt = T;
    bool unresolved = false;
    if (!aligned) unresolved = true;               // bring the early stoppers up to T, then look again
    else if (!all_good && T < cap) { tgt = T + 1; unresolved = true; }
    for (int f = f0; f < f1; f++) target[f] = tgt;
    if (unresolved) atomicAdd(flag, 1);
    else if (ret) ret[g] = all_good ? cap - T : -1;
}

// Hard decision + MSB-first packing (ldpc_decoder_bb_impl.cc:432-442) and optional soft output
// (the llr_pdu payload, :422-429), undoing the parity permutation (layered_decoder.hh:155-157).
// One thread per eight LLRs = one output byte. The information part of the state is in natural order: one 8-byte load, the
// sign bits gathered with a multiply (bits 7, 15, 23, 31 of a dword -> four adjacent bits), one byte stored (round 2 read
// byte by byte: 0.49 ms per 4096 normal frames, 1.3 % of a 50-update batch). The parity part (whole-codeword output and the
// soft output only) is gathered through the permutation pty[360 i + j] = parity[q j + i].
__device__ __forceinline__ uint32_t neg_bits4(uint32_t w) // offset-binary bytes b0..b3 -> (b0 < 0x80) << 3 | ... | (b3 < 0x80)
{
    const uint32_t m = (~w & 0x80808080u) >> 7;            // one bit per byte, at bits 0, 8, 16, 24
    return ((m * 0x08040201u) >> 24) & 0xfu;               // b0 -> bit 3, b1 -> bit 2, b2 -> bit 1, b3 -> bit 0
}
__global__ void ldpc_finalize_kernel(const uint8_t* state, uint8_t* bits, int8_t* llr_out,
                                     int N, int K, int q, int out_bytes)
{
    const int f = blockIdx.y;
    const uint8_t* s = state + (size_t)f * N;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= N / 8 || (!llr_out && b >= out_bytes)) return;
    uint2 v;
    if (8 * b < K) v = *reinterpret_cast<const uint2*>(s + 8 * b); // K % 8 == 0
    else {
        uint32_t w[2] = { 0, 0 };
        int r = 8 * b - K, jq = r / q, iq = r - jq * q;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            w[k >> 2] |= (uint32_t)s[K + kM * iq + jq] << (8 * (k & 3));
            if (++iq == q) { iq = 0; ++jq; }
        }
        v = make_uint2(w[0], w[1]);
    }
    if (llr_out) *reinterpret_cast<uint2*>(llr_out + (size_t)f * N + 8 * b) = make_uint2(v.x ^ 0x80808080u, v.y ^ 0x80808080u);
    if (bits && b < out_bytes) bits[(size_t)f * out_bytes + b] = (uint8_t)((neg_bits4(v.x) << 4) | neg_bits4(v.y));
}

// The per-CU pattern counters of the one-frame builds, ONE array per device for all handles (see the constructor): keyed by the device id,
// allocated on the CURRENT device and zeroed before its pointer is published, never freed (the counts survive the handles; they are not
// valid across hipDeviceReset()). A function of its own so that the table can be exercised with device keys a one-GPU box does not have
// (dvbs2_debug_cu_slot_table, tests/test_ldpc_gpu.py::test_cu_slot_table_is_per_device).
int* cu_slot_table(int device_key, std::string* err)
{
    static std::mutex mu;
    static std::vector<std::pair<int, int*>> per_device;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& e : per_device) if (e.first == device_key) return e.second;
    int* slots = nullptr;
    if (hipMalloc(&slots, kCuSlots * 4) != hipSuccess) { if (err) *err = "hipMalloc of the per-CU counters failed"; return nullptr; }
    if (hipMemset(slots, 0, kCuSlots * 4) != hipSuccess) { (void)hipFree(slots); if (err) *err = "hipMemset of the per-CU counters failed"; return nullptr; }
    per_device.push_back({ device_key, slots });
    return slots;
}

namespace {
// Environment overrides of the per-table choices below (the tests run every build on every table), read once per handle. Unset: the rule.
struct LdpcOverrides {
    std::optional<int> pr, pr_w1, pr_v2, dense, hz2, solo, soft_barrier, v2, v2p, group_sync, group_spin_max, resolve_rounds;
    bool timing = false; // DVBS2_TIMING: the cycle-stamped build and its printouts (diagnostics)
    LdpcOverrides()
    {
        auto get = [](const char* name) -> std::optional<int> { if (const char* e = getenv(name)) return atoi(e); return std::nullopt; };
        pr = get("DVBS2_PR"); pr_w1 = get("DVBS2_PR_W1"); pr_v2 = get("DVBS2_PR_V2"); dense = get("DVBS2_DENSE"); hz2 = get("DVBS2_HZ2");
        solo = get("DVBS2_SOLO"); soft_barrier = get("DVBS2_SOFT_BARRIER"); v2 = get("DVBS2_V2"); v2p = get("DVBS2_V2P");
        group_sync = get("DVBS2_GROUP_SYNC"); group_spin_max = get("DVBS2_GROUP_SPIN_MAX"); resolve_rounds = get("DVBS2_RESOLVE_ROUNDS");
        timing = getenv("DVBS2_TIMING") != nullptr;
    }
};
bool pick(const std::optional<int>& o, bool rule) { return o ? *o != 0 : rule; } // the override where one is set, else the rule

// The nearest pair (a, b) among the hazard entries of layer L (two entries of one group; distance d1 in rows) and the distance d2 of the
// next-nearest pair. The two-level walk (check_node_hazard) applies when the nearest pair is the layer's block and every other pair is at
// least twice as far apart -- the rows then go in outer blocks of d2 rows and only the near pair in ordered steps inside them.
struct NearPair { int a = -1, b = -1, d1 = 360, d2 = 360; bool two_level = false; };
NearPair nearest_pair(const LdpcSchedule& s, const LdpcLayer& L)
{
    NearPair p;
    for (int a = 0; a < L.n_conflict; a++)
        for (int b = a + 1; b < L.n_conflict; b++) {
            const LdpcEntry& ea = s.entries[L.entry_off + a], & eb = s.entries[L.entry_off + b];
            if (ea.base != eb.base) continue;
            const int d = std::abs((int)ea.rot - (int)eb.rot), dist = std::min(d, 360 - d);
            if (dist < p.d1) { p.d2 = p.d1; p.d1 = dist; p.a = a; p.b = b; }
            else p.d2 = std::min(p.d2, dist);
        }
    p.two_level = p.a >= 0 && p.d1 == L.block && p.d2 >= 2 * p.d1 && 360 / p.d1 - 360 / p.d2 >= 3;
    return p;
}

// the entry points of one sweep kernel family: the classic kernel per degree class (ldpc_inst_<dmax>.hip), parity in records (ldpc_inst_pr.hip)
struct SweepOps { hipError_t (*prepare)(LdpcBuild, size_t pair_lds_bytes, size_t solo_lds_bytes); void (*launch)(const LdpcLaunch&); };
hipError_t pr_prepare(LdpcBuild b, size_t lds_bytes, size_t) { return ldpc_pr_prepare(b, lds_bytes); }
const SweepOps& sweep_ops(bool pr, int dmax)
{
    static const SweepOps kPr = { pr_prepare, ldpc_pr_launch };
    static const SweepOps kClassic[8] = {
        { ldpc_variant_prepare<4>, ldpc_variant_launch<4> },   { ldpc_variant_prepare<8>, ldpc_variant_launch<8> },
        { ldpc_variant_prepare<12>, ldpc_variant_launch<12> }, { ldpc_variant_prepare<16>, ldpc_variant_launch<16> },
        { ldpc_variant_prepare<20>, ldpc_variant_launch<20> }, { ldpc_variant_prepare<24>, ldpc_variant_launch<24> },
        { ldpc_variant_prepare<28>, ldpc_variant_launch<28> }, { ldpc_variant_prepare<32>, ldpc_variant_launch<32> },
    };
    return pr ? kPr : kClassic[dmax / 4 - 1];
}
} // namespace

LdpcDecoderHip::LdpcDecoderHip(const LdpcTableDesc* table, int out_bits_message, int group_size, int max_frames, int device)
    : out_bits_message_(out_bits_message), G_(group_size), max_frames_(max_frames), device_(device)
{
    if (!compile_ldpc_schedule(table, &sched_)) { err_ = "unknown or inconsistent LDPC table"; return; }
    if (G_ < 1 || max_frames_ < 1 || max_frames_ > 65535) { err_ = "bad group_size/max_frames (max_frames 1..65535: frames are one launch dimension)"; return; }
    if (out_bits_message_ <= 0 || out_bits_message_ > sched_.N || out_bits_message_ % 8) { err_ = "bad message length"; return; }
    const LdpcOverrides ov;
    int degmax = 0, degmin = 1000;
    for (const LdpcLayer& L : sched_.layers) { degmax = std::max(degmax, L.cnt + 2); degmin = std::min(degmin, L.cnt + 2); }
    if (degmax > 32) { err_ = "check degree > 32 unsupported"; return; }
    // ---- which build of the sweep kernel (decided once, here, before the records are laid out for it) ----
    // "parity in records" variant (ldpc_kernel_pr.hpp): check degree <= 7, at most 4 hazard entries per layer, and two
    // pair workgroups must fit the 160 KB of LDS
    // Policy (measured on MI355X, tools/pr_sweep.sh; the two variants give identical bits): every eligible short and
    // medium table gains 12-43 % from the second workgroup per CU. On normal frames the classic kernel is as fast or
    // faster since its hazard layers run as lane chains (B4: 109 k vs 106 k frames/s; thin-layer tables lose up to
    // 20 % with parity-in-records).
    // Round 6: also the two NORMAL tables of check degree <= 4 (1/4 normal, S2X 2/9 normal: one-dword records, four frames per CU): interleaved A/B
    // 154.1 -> 158.9 k and 152.8 -> 157.6 k frames/s (+3.1 %); the other normal tables of degree <= 7 lose with it (2/5 0.958, B4 0.989, 1/3 0.941, S2X 13/45 0.849).
    pr_ = degmax <= 7 && pick(ov.pr, sched_.N < 64800 || degmax <= 4);
    for (const LdpcLayer& L : sched_.layers)
        if (L.block < 360 && (L.n_conflict > 4 || (L.n_conflict > 2 ? 4 : 2) > L.cnt)) pr_ = false;
    pr_shared_sv_ = 2 * pr_lds_bytes(sched_.N, sched_.K) > 160 * 1024; // (normal frames forced onto this kernel: one sign-vector area per workgroup)
    if (2 * pr_lds_bytes(sched_.N, sched_.K, pr_shared_sv_) > 160 * 1024) pr_ = false;
    // degree class: the sweep kernel is built per multiple of four (message dwords per check); degree <= 4 tables that do not run the
    // parity-in-records kernel (1/4 normal, S2X 2/9 normal) get the one-dword class -- they move ~4.4 TB/s with two (+8 %)
    dmax_ = pr_ ? 8 : std::max(4, (degmax + 3) / 4 * 4);
    if (degmin < 3 || degmin <= dmax_ - 8) { err_ = "check degree spread unsupported by the kernel variants"; return; }
    words_per_check_ = dmax_ / 4;
    // Short frames whose layers are mostly hazard layers (latency-bound ordered steps) and whose degree rules out the
    // parity-in-records kernel: the 80-VGPR build puts a second workgroup on the CU (measured: short 3/5 and 2/3 +34 %;
    // it costs 6-18 % where regular layers dominate, hence the 70 % threshold; degree classes above 12 do not fit 80 VGPRs).
    // It has no two-level lane chain (76 -> 349 spilled registers, round 3) and, since round 4, no single-pair lane chain either -- with
    // its tables addressed as LDS (typed pointers, ldpc_kernel.hpp) the chain code made that build spill ten times as much (72 -> 725)
    // and short 3/5 / 2/3 lost 30 %; its layers take the block scheme.
    const bool dense = !pr_ && dmax_ == 12 && 4 * half_lds_bytes(sched_.N) <= 160 * 1024 &&
                       pick(ov.dense, sched_.N < 64800 && 10 * sched_.conflict_layers >= 7 * sched_.q);
    // Which of the other builds: measured per table (ldpc_policy.inc <- tools/policy_sweep.py + tools/gen_policy.py); a table
    // that is not listed takes the plain pair kernel.
    bool pol_packed = false, pol_solo = false;
    {
        struct Pol { const char* table; int packed, solo; };
        static const Pol kPolicy[] = {
#include "ldpc_policy.inc"
        };
        for (const Pol& p : kPolicy) if (!strcmp(p.table, table->name)) { pol_packed = p.packed; pol_solo = p.solo; }
    }
    // The build with the heavy-hazard paths (HZ2: up to twelve ordered entries per check instead of the one-wave walk, two-level walk
    // where one hazard pair is much closer than the rest): tables listed in ldpc_policy_hz2.inc (measured, tools/hz2_sweep.sh).
    bool pol_hz2 = false;
    {
        static const char* const kHz2[] = {
#include "ldpc_policy_hz2.inc"
        };
        for (const char* n : kHz2) if (!strcmp(n, table->name)) pol_hz2 = true;
    }
    const bool hz2 = !dense && dmax_ >= 12 && pick(ov.hz2, pol_hz2);
    const bool solo = !pr_ && !dense && !hz2 && dmax_ <= kSoloMaxDmax && !ov.timing && pick(ov.solo, pol_solo);
    // frame barriers in software (ldpc_kernel.hpp): by rule where no layer has hazards; with hazard layers only for the tables listed in
    // ldpc_policy_soft.inc (measured on two leases, tools/soft_sweep.py)
    bool pol_soft = sched_.conflict_layers == 0;
    {
        static const char* const kSoft[] = {
#include "ldpc_policy_soft.inc"
        };
        for (const char* n : kSoft) if (!strcmp(n, table->name)) pol_soft = true;
    }
    const bool soft_bar = !pr_ && !dense && !solo && !hz2 && !ov.timing && dmax_ >= 20 && pick(ov.soft_barrier, pol_soft); // (built for the degree classes >= 20)
    // the packed build is the table's policy or forced; the fit test below may still send the table to the plain build
    bool packed = !pr_ && !dense && !hz2 && pick(ov.v2, pol_packed);
    const bool v2p_on = pick(ov.v2p, true); // hazard layers with the packed first / last phase (classes v2p_class); DVBS2_V2P=0: tests
    // one-dword records (four 6-bit messages + the parity byte, ldpc_kernel_pr.hpp): check degree <= 4
    const bool pr_w1 = pr_ && degmax <= 4 && pick(ov.pr_w1, true);
    if (pr_w1) words_per_check_ = 1;
    // packed nodes (check_node_v2_pr) in the regular middle layers of the two-dword-record kernel: per-wave sweep records as for the classic packed builds
    // Measured (MI355X, interleaved A/B x 3): short 2/5, 1/2, S2X short 26/45 / medium 1/3 +3.0 ... +3.8 %, short 1/3 +0.7 %; on NORMAL frames forced onto
    // this kernel (DVBS2_PR=1) B4 +2.1 % and S2X 9/20 +2.5 % on never-converging input -- and B4 9 % SLOWER at its operating point (Es/N0 2.0 dB: 353 -> 323 k frames/s;
    // this kernel's full syndrome test fetches the parity signs from the records): short / medium frames by rule, normal frames stay with the classic builds.
    const bool pr_v2 = pr_ && !pr_w1 && pick(ov.pr_v2, sched_.N < 64800);

    DeviceGuard dev_guard(device_); // the caller's current device is restored when the constructor returns (device_guard.h)
    if (!dev_guard.ok) { err_ = "hipSetDevice failed"; return; }
    const int RS = rec_stride(dmax_);
    std::vector<uint32_t> hr((size_t)sched_.q * RS, 0);
    std::vector<std::vector<int>> layer_order(sched_.q); // record order of every layer's entries (ordered entries first, host-oriented pairs)
    std::vector<int> layer_nc(sched_.q, 0);              // ordered entries the kernel handles in the layer's ordered phase (2, 4, 8, 12; kHazardWalk)
    for (int i = 0; i < sched_.q; i++) {
        const LdpcLayer& L = sched_.layers[i];
        uint32_t nc_code = 0;
        if (L.block < 360) {
            nc_code = L.n_conflict <= 2 ? 2 : L.n_conflict <= 4 ? 4 : L.n_conflict <= 8 ? 8 : 12;
            if (L.n_conflict > (hz2 && dmax_ <= kMaxHazard12Dmax ? kMaxHazardHz2 : kMaxHazard) || (int)nc_code > L.cnt) nc_code = kHazardWalk;
        }
        // A layer whose only hazard is ONE pair (two entries of one group) with a small block is walked as a lane
        // chain (check_node_hazard): the pair is ordered so that entry 0's bit of row j is entry 1's bit of row
        // j + block, i.e. (rot0 - rot1) mod 360 == block; header bit 12. Needs lane_chain_words(block) of scratch per
        // frame in the sign-vector area. (Rounds 2-3, integer walk: gains up to block 64, flat to 128, slightly negative at 180; round 4,
        // float walk and packed chain: +0.2...1.6 % at 180.)
        int order[64];
        for (int k = 0; k < L.cnt + 2; k++) order[k] = k;
        uint32_t chain = 0;
        if (!dense && L.block <= kChainMaxBlock && nc_code == 2 && L.n_conflict == 2 && (L.cnt + 2 <= kLaneChainMaxDeg || (packed && v2p_class(dmax_))) &&
            (sched_.N / 360) * kSvWords >= lane_chain_words(L.block)) {
            const LdpcEntry& a = sched_.entries[L.entry_off], & b = sched_.entries[L.entry_off + 1];
            if (a.base == b.base) {
                const int D = ((int)a.rot - (int)b.rot + 360) % 360;
                if (D == L.block) chain = 1;
                else if (360 - D == L.block) { order[0] = 1; order[1] = 0; chain = 1; }
            }
        }
        // Two-level walk (check_node_hazard, nearest_pair): the near pair goes first (entries 0, 1); word 2 of the record = the distance
        // of the nearest OTHER pair = rows per outer block.
        uint32_t block2 = 0;
        auto near_pair_first = [&](const NearPair& p) {
            block2 = (uint32_t)p.d2;
            order[0] = p.a; order[1] = p.b;
            int n = 2;
            for (int k = 0; k < L.n_conflict; k++) if (k != p.a && k != p.b) order[n++] = k;
        };
        // (the degree class 32 without the heavy-hazard paths walks the near pair as a lane chain inside the outer blocks -- the
        // two-level lane chain of check_node_hazard: the pair additionally has to be oriented like a single-pair chain, bit 12;
        // not in the 80-VGPR build: the chain's state does not fit there, 76 -> 349 spilled registers)
        const bool tlc_build = tlc_class(dmax_) && !hz2 && !pr_ && !dense && !soft_bar; // (kTlc<DMAX, HZ2> && !SOFT && MINW == 1 in the kernel)
        if (tlc_build && L.block < 360 && L.block <= kChainMaxBlock && (nc_code == 4 || nc_code == 8) &&
            (sched_.N / 360) * kSvWords >= lane_chain_words(L.block)) {
            NearPair p = nearest_pair(sched_, L);
            if (p.two_level) {
                const int D = ((int)sched_.entries[L.entry_off + p.a].rot - (int)sched_.entries[L.entry_off + p.b].rot + 360) % 360;
                if (D != L.block) std::swap(p.a, p.b); // entry 0's bit of row r = entry 1's bit of row r + block  <=>  (rot0 - rot1) mod 360 == block
                chain = 1;
                near_pair_first(p);
            }
        }
        if (hz2 && L.block < 360 && nc_code >= 4 && nc_code != (uint32_t)kHazardWalk && (L.cnt + 2 < 29 || nc_code == 8)) {
            const NearPair p = nearest_pair(sched_, L);
            if (p.two_level) near_pair_first(p);
        }
        layer_order[i].assign(order, order + L.cnt + 2);
        layer_nc[i] = (int)nc_code;
        hr[(size_t)i * RS] = L.cnt | (nc_code << 8) | (chain << 12) | ((uint32_t)L.sync_before << 15) | ((uint32_t)L.block << 16);
        hr[(size_t)i * RS + 2] = block2;
        for (int k = 0; k < L.cnt + 2; k++) {
            const LdpcEntry& e = sched_.entries[L.entry_off + order[k]];
            hr[(size_t)i * RS + 4 + 2 * k] = (uint32_t)e.base + e.rot;
            hr[(size_t)i * RS + 5 + 2 * k] = 360u - e.rot;
        }
    }
    if (pr_) for (int i = 0; i < sched_.q; i++) hr[(size_t)i * RS] &= ~(1u << 12); // that kernel has no lane chain (80 VGPRs)
    if (pr_) {
        const int q = sched_.q;
        hr[(size_t)(q - 1) * RS + 4 + 2 * sched_.layers[q - 1].cnt] = (uint32_t)sched_.K;          // own parity of the last layer: row q-1 at offset K
        hr[(size_t)(q - 1) * RS + 5 + 2 * sched_.layers[q - 1].cnt] = 360u;
        hr[(size_t)0 * RS + 4 + 2 * (sched_.layers[0].cnt + 1)] = (uint32_t)sched_.K + 359u;     // previous parity of layer 0: same row, one lane down
        hr[(size_t)0 * RS + 5 + 2 * (sched_.layers[0].cnt + 1)] = 1u;
    }
    HIP_OK(hipMalloc(&d_recs_alloc_, (hr.size() + kRecHeaderWords) * 4)); // header (group-synchronous stop, filled below) + records
    d_recs_ = d_recs_alloc_ + kRecHeaderWords;
    HIP_OK(hipMemcpy(d_recs_, hr.data(), hr.size() * 4, hipMemcpyHostToDevice));
    // Sweep records per (layer, wave) for the classic kernel (check_node_v2 in ldpc_kernel.hpp). A regular layer i > 0 gets,
    // for each of the six waves of a frame, its data entries reordered "mixed first" (mixed = the wrap point 360 - rot lies
    // inside the wave's rows), window offsets pre-adjusted for the wave, and the lane masks of the mixed entries; a wave
    // with more mixed entries than fix slots, layer 0 and hazard layers keep the classic record (replicated).
    // "Pure" packed builds (ldpc_kernel.hpp, kPure: the packed builds of the degree class 32): the plain nodes exist for layer 0
    // only, so EVERY (layer > 0, wave) record has to fit the packed format -- mixed entries within the fix slots, no one-wave walk layer. A
    // table that does not fit takes the plain build (of the 57 tables this concerns 9/10 normal only, which fits).
    if (packed && v2_pure_class(dmax_)) {
        bool fits = v2p_on;
        for (int i = 1; fits && i < sched_.q; i++) {
            const LdpcLayer& L = sched_.layers[i];
            const int ncv = layer_nc[i];
            if (L.block < 360 && !((ncv == 2 || ncv == 4 || ncv == 8) && (int)L.cnt >= ncv && v2p_class(dmax_))) { fits = false; break; }
            for (int w = 0; w < 6 && fits; w++) {
                const int lo = 64 * w, hi = std::min(64 * w + 63, 359);
                int nm = 0;
                for (int k = L.block < 360 ? ncv : 0; k < L.cnt; k++) { const int thr = 360 - (int)sched_.entries[L.entry_off + layer_order[i][k]].rot; nm += lo < thr && thr <= hi; }
                if (nm > (L.block < 360 ? std::min(dmax_ / 2, (int)L.cnt) - ncv : std::min(v2_nfix(dmax_), (int)L.cnt))) fits = false;
            }
        }
        if (!fits) packed = false;
    }
    const int RSW = rec_stride_wave(dmax_);
    std::vector<uint32_t> wr((size_t)sched_.q * 6 * RSW, 0);
    // single-pair hazard layers walked by the packed register chain (check_node_chain_v2, built for the degree classes <= 16): block <=
    // kChainMaxBlock, the pair are the first two entries (schedule compiler), and on every wave the mixed regular entries fit the fix slots after the pair's
    std::vector<char> chain_v2_layer(sched_.q, 0), chain_order(sched_.q, 0);
    for (int i = 1; packed && dmax_ <= 16 && i < sched_.q; i++) {
        const LdpcLayer& L = sched_.layers[i];
        if (L.block >= 360 || L.block > kChainMaxBlock || L.n_conflict != 2 || L.cnt < 2) continue;
        const LdpcEntry& a = sched_.entries[L.entry_off], & b = sched_.entries[L.entry_off + 1];
        if (a.base != b.base) continue;
        const int D = ((int)a.rot - (int)b.rot + 360) % 360; // X's bit of row r is Y's bit of row r + block  <=>  (rotX - rotY) mod 360 == block
        if (D == L.block) chain_order[i] = 0; else if (360 - D == L.block) chain_order[i] = 1; else continue;
        bool fits = true;
        for (int w = 0; w < 6; w++) {
            const int lo = 64 * w, hi = std::min(64 * w + 63, 359);
            int nm = 0;
            for (int k = 2; k < L.cnt; k++) { const int thr = 360 - (int)sched_.entries[L.entry_off + k].rot; nm += lo < thr && thr <= hi; }
            if (nm > v2_nfix(dmax_)) fits = false;
        }
        chain_v2_layer[i] = fits;
    }
    for (int i = 0; i < sched_.q; i++) {
        const LdpcLayer& L = sched_.layers[i];
        for (int w = 0; w < 6; w++) {
            uint32_t* rec = &wr[((size_t)i * 6 + w) * RSW];
            std::copy(hr.begin() + (size_t)i * RS, hr.begin() + (size_t)(i + 1) * RS, rec);
            if (i == 0) continue;
            const bool chain2 = L.block < 360 && chain_v2_layer[i];
            // hazard layers of the packed builds whose ordered phase is the generic one (check_node_hazard<..., V2P>, ldpc_kernel.hpp): the NC
            // ordered entries keep their record order in the first fix slots, the mixed regular entries follow; dmax / 2 fix slots in all
            const int ncv = layer_nc[i];
            const bool v2p = packed && v2p_on && v2p_class(dmax_) && L.block < 360 && !chain2 && (ncv == 2 || ncv == 4 || ncv == 8) && (int)L.cnt >= ncv;
            // (parity-in-records: the last layer keeps its plain node, like layer 0; check_node_v2_pr exists for the degrees 5 .. 7)
            if (L.block < 360 ? !(chain2 || v2p) : !(packed || (pr_v2 && i != sched_.q - 1 && L.cnt + 2 >= 5))) continue;
            const int lo = 64 * w, hi = std::min(64 * w + 63, 359);
            std::vector<int> mixed, plain;
            auto is_mixed = [&](int k) { const int thr = 360 - (int)sched_.entries[L.entry_off + k].rot; return lo < thr && thr <= hi; };
            if (v2p) { for (int k = ncv; k < L.cnt; k++) { const int e = layer_order[i][k]; (is_mixed(e) ? mixed : plain).push_back(e); } }
            else for (int k = chain2 ? 2 : 0; k < L.cnt; k++) (is_mixed(k) ? mixed : plain).push_back(k);
            const int nfix = v2p ? std::min(dmax_ / 2, (int)L.cnt) - ncv : std::min(v2_nfix(dmax_), (int)L.cnt);
            if (!chain2 && (int)mixed.size() > nfix) continue; // (a chain layer was checked for every wave beforehand)
            std::fill(rec + 4, rec + RSW, 0u);
            rec[0] = hr[(size_t)i * RS] | (1u << 13) | (v2p ? 1u << 14 : 0u);
            int slot = 0;
            auto put = [&](int k, bool is_mixed) {
                const LdpcEntry& e = sched_.entries[L.entry_off + k];
                const int thr = 360 - (int)e.rot;
                const uint32_t S0 = (uint32_t)e.base + e.rot;
                uint32_t off = S0;                       // every row of the wave below the wrap point
                if (is_mixed || lo >= thr) off = S0 - 360u; // wrapped (mixed: the lanes below the wrap point get + 360 back)
                rec[4 + slot] = off;
                if (is_mixed) {
                    unsigned long long m = 0;
                    for (int l = 0; l < 64; l++) if (std::min(lo + l, 359) < thr) m |= 1ull << l; // threads 360..383 mirror row 359
                    rec[4 + dmax_ + 2 * slot] = (uint32_t)m; rec[4 + dmax_ + 2 * slot + 1] = (uint32_t)(m >> 32);
                }
                slot++;
            };
            if (chain2) { // the pair X, Y (host-ordered: hr already holds them in chain order) takes the first two fix slots
                const int kx = chain_order[i] ? 1 : 0;
                put(kx, is_mixed(kx)); put(1 - kx, is_mixed(1 - kx));
            }
            if (v2p) for (int k = 0; k < ncv; k++) { const int e = layer_order[i][k]; put(e, is_mixed(e)); } // ordered entries, in the per-layer record's order
            for (int k : mixed) put(k, true);
            for (int k : plain) put(k, false);
            put(L.cnt, false);     // own parity (rot 0)
            put(L.cnt + 1, false); // previous parity (rot 0 for i > 0)
        }
    }
    // "Pure" packed builds have no plain node for layers > 0: a (layer, wave) record that is NOT in the packed format would do no work there and
    // the decode would be silently wrong. The `fits` predicate above is a second copy of the record builder's rules: check the
    // records that were actually BUILT, and refuse the table loudly instead of trusting the copy.
    if (packed && v2_pure_class(dmax_)) {
        for (int i = 1; i < sched_.q; i++)
            for (int w = 0; w < 6; w++) {
                const uint32_t h0 = wr[((size_t)i * 6 + w) * RSW];
                const bool hazard = sched_.layers[i].block < 360;
                if (!((h0 >> 13) & 1u) || (hazard && !((h0 >> 14) & 1u))) {
                    err_ = "internal: a (layer, wave) record of a pure packed build is not in the packed format (layer " + std::to_string(i) + ", wave " + std::to_string(w) + ")";
                    return;
                }
            }
    }
    if (pr_) build_ = pr_w1 ? LdpcBuild::pr_w1 : pr_v2 ? LdpcBuild::pr_packed : LdpcBuild::pr;
    else if (dense) build_ = LdpcBuild::dense;
    else if (hz2) build_ = LdpcBuild::hz2;
    else if (soft_bar) build_ = packed ? LdpcBuild::packed_soft : LdpcBuild::soft;
    else if (solo) build_ = packed ? LdpcBuild::packed_solo : LdpcBuild::solo;
    else build_ = packed ? LdpcBuild::packed : LdpcBuild::plain;
    HIP_OK(hipMalloc(&d_wrecs_, wr.size() * 4));
    HIP_OK(hipMemcpy(d_wrecs_, wr.data(), wr.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d_state_, (size_t)max_frames_ * sched_.N));
    HIP_OK(hipMalloc(&d_msgs_, (size_t)max_frames_ * sched_.q * words_per_check_ * kMsgStride * 4));
    HIP_OK(hipMalloc(&d_iters_, (size_t)max_frames_ * 4));
    HIP_OK(hipMalloc(&d_good_, (size_t)max_frames_ * 4));
    HIP_OK(hipMalloc(&d_target_, (size_t)max_frames_ * 4));
    // Group-synchronous stop (ldpc_kernel.hpp, group_decide): the frames of a group agree after every syndrome test, so the whole
    // group stops at the reference's count inside the first pass and the resolution rounds have nothing left to do (they stay as
    // the fallback; with the rule on, none is enqueued ahead of time). Needs the members of a group resident together: groups of up
    // to 64 frames (at most 32 pair workgroups of 256 CUs). DVBS2_GROUP_SYNC=0 / 1 overrides (tests run both).
    gsync_on_ = G_ <= 64 && pick(ov.group_sync, true);
    if (gsync_on_) {
        HIP_OK(hipMalloc(&d_gsync_, (size_t)(max_frames_ + 64) * 4)); // one status word per frame (group_decide)
        resolve_rounds_ = 0;
        const unsigned long long a = (unsigned long long)d_iters_, b = (unsigned long long)d_gsync_;
        const int spin_max = ov.group_spin_max ? std::max(0, *ov.group_spin_max) : kGroupSpinMax; // tests: 0 = a waiting member gives up at once (fallback path)
        const uint32_t hd[kRecHeaderWords] = { (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)G_, (uint32_t)spin_max, 0, 0 };
        HIP_OK(hipMemcpy(d_recs_alloc_, hd, sizeof(hd), hipMemcpyHostToDevice));
    }
    if (ov.resolve_rounds) resolve_rounds_ = std::max(0, std::min(8, *ov.resolve_rounds)); // tests: 0 forces the host-side leftover path
    HIP_OK(hipMalloc(&d_flag_, 4 * kSlots));
    HIP_OK(hipHostMalloc(&h_flag_, 4 * kSlots));
    HIP_OK(hipEventCreate(&ev0_));
    HIP_OK(hipEventCreate(&ev1_));
    if (ov.timing) { HIP_OK(hipMalloc(&d_tdbg_, ((size_t)max_frames_ * 48 + 512) * 8)); HIP_OK(hipMemset(d_tdbg_, 0, ((size_t)max_frames_ * 48 + 512) * 8)); }
    if (is_solo(build_)) {
        // The per-CU pattern counters of the one-frame builds are shared by ALL handles of a device: two workgroups on a CU take
        // complementary wave patterns through them, whichever launch (handle, stream) they belong to. With one array per handle two
        // pipelined handles both chose pattern 0 on every CU: 4,4,2,2 working waves per SIMD instead of 3,3,3,3 and the operating point
        // through two handles fell from 0.92 to 0.71 of the proportional rate (round 4). Allocated once per device, never freed.
        // Keyed by the device this constructor actually runs on (hipGetDevice behind the guard), one entry per device ever seen; the
        // array is zeroed BEFORE its pointer is published. The counts survive the handles (a kernel gives its slot back when it ends);
        // they are not valid across hipDeviceReset().
        int dv = -1;
        HIP_OK(hipGetDevice(&dv));
        std::string e;
        int* slots = cu_slot_table(dv, &e);
        if (!slots) { err_ = e; return; }
        d_cu_slots_ = slots;
    }
    static const char* const kSuffix[kLdpcBuilds] = { ">", ", packed>", ", solo>", ", packed, solo>", ", hz2>", ", soft>", ", packed, soft>", ", dense>",
                                                      "", "<w1>", "<packed>" };
    kname_ = std::string(pr_ ? "ldpc_layered_pr_kernel" : "ldpc_layered_kernel<" + std::to_string(dmax_)) + kSuffix[(int)build_];
    lds_bytes_ = pr_ ? pr_lds_bytes(sched_.N, sched_.K, pr_shared_sv_) : 2 * half_lds_bytes(sched_.N);
    HIP_OK(sweep_ops(pr_, dmax_).prepare(build_, lds_bytes_, half_lds_bytes(sched_.N)));
}

LdpcDecoderHip::~LdpcDecoderHip()
{
    DeviceGuard dev_guard(device_);
    (void)hipFree(d_recs_alloc_); (void)hipFree(d_wrecs_); (void)hipFree(d_state_); (void)hipFree(d_msgs_);
    (void)hipFree(d_iters_); (void)hipFree(d_good_); (void)hipFree(d_target_); (void)hipFree(d_flag_); (void)hipFree(d_gsync_);
    if (h_flag_) (void)hipHostFree(h_flag_);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
}

void LdpcDecoderHip::launch_sweep(const int8_t* in, bool resume, int stop_on_good, int n_frames, int max_trials, int frame_base, hipStream_t stream, const DemapFused* dm)
{
    if (profiling_) (void)hipEventRecord(ev0_, stream);
    const size_t fb = (size_t)frame_base;
    LdpcLaunch la;
    la.recs = d_recs_; la.wrecs = d_wrecs_; la.llr_in = in; la.state = d_state_ + fb * sched_.N;
    la.msgs = d_msgs_ + fb * sched_.q * words_per_check_ * kMsgStride;
    la.iters = d_iters_ + fb; la.good = d_good_ + fb; la.target = resume ? d_target_ + fb : nullptr;
    const bool gs = gsync_on_ && !resume && stop_on_good; // group-synchronous stop: bit 2 of the flag word; its words start from zero
    if (gs) (void)hipMemsetAsync(d_gsync_ + frame_base, 0, (size_t)n_frames * 4, stream); // (frame_base is a multiple of the group size: enqueue())
    const bool soft_bar = build_ == LdpcBuild::soft || build_ == LdpcBuild::packed_soft;
    la.n_frames = n_frames; la.N = sched_.N; la.K = sched_.K; la.q = sched_.q; la.cap = max_trials; la.stop_on_good = stop_on_good | (soft_bar ? 2 : 0) | (gs ? 4 : 0) | (pr_ && pr_shared_sv_ ? 8 : 0);
    la.tdbg = d_tdbg_; la.lds_bytes = is_solo(build_) ? half_lds_bytes(sched_.N) : lds_bytes_; la.stream = stream;
    la.build = build_; la.cu_slots = d_cu_slots_;
    la.dm = DemapFused{};
    if (dm && !resume) la.dm = *dm;
    sweep_ops(pr_, dmax_).launch(la);
    if (profiling_ && !resume) { // the first pass is the dominant launch; timing it serialises the stream (bench.py's roofline leg only)
        (void)hipEventRecord(ev1_, stream);
        (void)hipEventSynchronize(ev1_);
        float ms = 0; (void)hipEventElapsedTime(&ms, ev0_, ev1_);
        prof_ms_ += ms; prof_launches_++;
    }
}

void LdpcDecoderHip::launch_targets(int n_frames, int max_trials, int frame_base, int32_t* d_ret, int slot, hipStream_t stream)
{
    const int n_groups = (n_frames + G_ - 1) / G_;
    (void)hipMemsetAsync(d_flag_ + slot, 0, 4, stream);
    hipLaunchKernelGGL(ldpc_group_targets_kernel, dim3((n_groups + 127) / 128), dim3(128), 0, stream,
                       d_iters_ + frame_base, d_good_ + frame_base, d_target_ + frame_base, d_flag_ + slot, d_ret, n_groups, G_, n_frames, max_trials);
}

void LdpcDecoderHip::launch_finalize(const Pending& p)
{
    if (!p.bits && !p.llr_out) return; // nobody asked for packed bits or LLRs (chain: the BCH stage reads the state)
    const int out_bytes = (p.out_mode ? out_bits_message_ : sched_.N) / 8;
    const int items = p.llr_out ? sched_.N / 8 : out_bytes; // one thread per eight LLRs; without the soft output only the bytes asked for
    hipLaunchKernelGGL(ldpc_finalize_kernel, dim3((items + 255) / 256, p.n_frames), dim3(256), 0, p.stream,
                       d_state_ + (size_t)p.frame_base * sched_.N, p.bits, p.llr_out, sched_.N, sched_.K, sched_.q, out_bytes);
}

int LdpcDecoderHip::enqueue(const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode, uint8_t* d_bits_out, int8_t* d_llr_out,
                            int32_t* d_ret, hipStream_t stream, int slot, int frame_base, const DemapFused* dm)
{
    if (!ok()) return -1;
    call_err_.clear();
    if (slot < 0 || slot >= kSlots) { call_err_ = "bad slot"; return -1; }
    if (pend_[slot].active) { call_err_ = "slot busy: finish() the previous decode first"; return -1; }
    if (n_frames < 0 || frame_base < 0 || frame_base + n_frames > max_frames_) { call_err_ = "n_frames exceeds max_frames"; return -1; }
    if (frame_base % 2 || (frame_base && frame_base % G_)) { call_err_ = "frame_base must be a multiple of the group size and even"; return -1; }
    if (max_trials < 0) { call_err_ = "max_trials < 0"; return -1; }
    Pending& p = pend_[slot];
    // a call that fails below leaves the slot free again (the handle stays usable: "a failed call does not disable the handle")
    // (and nothing of it stays in flight: kernels and copies already queued on the stream are waited for before the slot is given up)
    struct Release { Pending& p; bool armed = true, launched = false; ~Release() { if (armed) { if (launched) (void)hipStreamSynchronize(p.stream); p.active = false; } } } release{ p };
    p.active = true; p.n_frames = n_frames; p.max_trials = max_trials; p.out_mode = out_mode; p.frame_base = frame_base;
    p.bits = d_bits_out; p.llr_out = d_llr_out; p.ret = d_ret; p.stream = stream;
    h_flag_[slot] = 0;
    if (n_frames == 0) { release.armed = false; return 0; }
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { call_err_ = "hipSetDevice failed"; return -1; }
    if (dm && dm->mode && pr_) { call_err_ = "this sweep kernel does not demap while loading"; return -1; }
    release.launched = true;
    launch_sweep(d_llr_in, false, 1, n_frames, max_trials, frame_base, stream, dm);
    if (d_tdbg_) {
        HIP_RET(hipStreamSynchronize(stream));
        if (getenv("DVBS2_TIMING_LAYERS")) { // cycles per layer of frame 0, wave 0 (sum over the sweeps so far)
            std::vector<unsigned long long> hl(sched_.q);
            HIP_RET(hipMemcpy(hl.data(), d_tdbg_ + (size_t)n_frames * 48, hl.size() * 8, hipMemcpyDeviceToHost));
            {   // hazard-node phases (check_node_hazard, DVBS2_PH): wave 0 = chain heads / walker, wave 5 = body rows
                std::vector<unsigned long long> hp(32);
                HIP_RET(hipMemcpy(hp.data(), d_tdbg_ + (size_t)n_frames * 48 + 256, 32 * 8, hipMemcpyDeviceToHost));
                static const char* const nm[8] = { "P1", "heads", "barrier", "publish+barrier", "walk", "barrier", "steps/finish+barrier", "merge+P3" };
                for (int w = 0; w < 2; w++) {
                    fprintf(stderr, "  hazard phases wave %d (cycles/sweep):", w ? 5 : 0);
                    for (int k = 0; k < 8; k++) fprintf(stderr, " %s %.0f", nm[k], (double)hp[16 * w + k] / std::max(1, max_trials));
                    fprintf(stderr, "\n");
                }
            }
            HIP_RET(hipMemset(d_tdbg_ + (size_t)n_frames * 48, 0, 512 * 8));
            for (int i = 0; i < sched_.q; i++) fprintf(stderr, "  layer %3d block %3d nconf %d deg %2d: %8.0f cycles/sweep\n", i, sched_.layers[i].block, sched_.layers[i].n_conflict, sched_.layers[i].cnt + 2, (double)hl[i] / std::max(1, max_trials));
        }
        std::vector<unsigned long long> h((size_t)n_frames * 48);
        HIP_RET(hipMemcpy(h.data(), d_tdbg_, h.size() * 8, hipMemcpyDeviceToHost));
        double a[8] = {0};
        for (size_t r = 0; r < (size_t)n_frames * 6; r++) for (int c = 0; c < 8; c++) a[c] += (double)h[r * 8 + c];
        const double nr = (double)n_frames * 6;
        if (getenv("DVBS2_TIMING_WAVES")) {
            for (int w = 0; w < 6; w++) {
                double b[8] = {0};
                for (size_t fr = 0; fr < (size_t)n_frames; fr++) for (int c = 0; c < 8; c++) b[c] += (double)h[(fr * 6 + w) * 8 + c];
                fprintf(stderr, "  wave %d: sweep %.0f barrier %.0f body %.0f conflict %.0f\n", w, b[2] / n_frames, b[3] / n_frames, b[4] / n_frames, b[5] / n_frames);
            }
        }
        fprintf(stderr, "[timing, shader-clock cycles per wave avg] load %.0f synd %.0f sweep %.0f (barrier %.0f body %.0f conflict-layers %.0f) iters %.1f synd-step1 %.0f\n", a[0]/nr, a[1]/nr, a[2]/nr, a[3]/nr, a[4]/nr, a[5]/nr, a[6]/nr, a[7]/nr);
    }
    // group resolution on the device: no host round trip (a resume launch whose frames are all at their target costs a few
    // microseconds: its workgroups read two counters and leave)
    for (int r = 0; r < resolve_rounds_; r++) {
        launch_targets(n_frames, max_trials, frame_base, d_ret, slot, stream);
        launch_sweep(nullptr, true, 0, n_frames, max_trials, frame_base, stream);
    }
    launch_targets(n_frames, max_trials, frame_base, d_ret, slot, stream);
    launch_finalize(p);
    HIP_RET(hipMemcpyAsync(h_flag_ + slot, d_flag_ + slot, 4, hipMemcpyDeviceToHost, stream));
    HIP_RET(hipGetLastError());
    release.armed = false;
    return 0;
}

int LdpcDecoderHip::finish(int slot)
{
    if (!ok()) return -1;
    if (slot < 0 || slot >= kSlots) { call_err_ = "bad slot"; return -1; }
    Pending& p = pend_[slot];
    if (!p.active) return 0;
    p.active = false;
    if (p.n_frames == 0) return 0;
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { call_err_ = "hipSetDevice failed"; return -1; }
    HIP_RET(hipStreamSynchronize(p.stream));
    if (h_flag_[slot] == 0) return 0;
    struct Drain { hipStream_t st; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(st); } } drain{ p.stream }; // a failing round leaves nothing in flight
    for (int round = 0; h_flag_[slot] != 0; round++) { // the rare leftovers, one host round trip each
        if (round > 2 * p.max_trials + 2) { call_err_ = "group resolution did not converge"; return -1; }
        fallback_rounds_++;
        launch_sweep(nullptr, true, 0, p.n_frames, p.max_trials, p.frame_base, p.stream);
        launch_targets(p.n_frames, p.max_trials, p.frame_base, p.ret, slot, p.stream);
        HIP_RET(hipMemcpyAsync(h_flag_ + slot, d_flag_ + slot, 4, hipMemcpyDeviceToHost, p.stream));
        HIP_RET(hipStreamSynchronize(p.stream));
    }
    launch_finalize(p);
    HIP_RET(hipGetLastError());
    HIP_RET(hipStreamSynchronize(p.stream));
    drain.armed = false;
    return 1; // outputs were rewritten after the stream's first completion
}

void LdpcDecoderHip::abort_all()
{
    DeviceGuard dev_guard(device_);
    for (Pending& p : pend_) {
        if (p.active && p.n_frames > 0 && dev_guard.ok) (void)hipStreamSynchronize(p.stream);
        p.active = false;
    }
}

int LdpcDecoderHip::decode_device(const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode,
                                  uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret, hipStream_t stream)
{
    if (enqueue(d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, d_ret, stream, 0, 0)) return -1;
    return finish(0) < 0 ? -1 : 0;
}

} // namespace dvbs2
