// ldpc_plan.cpp -- see ldpc_plan.h. Three steps: choose the build (select_build), lay out the per-layer records (layer_records) and
// the per-(layer, wave) records (wave_records) for it.
#include "ldpc_plan.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace dvbs2 {

LdpcOverrides LdpcOverrides::from_env()
{
    auto get = [](const char* name) -> std::optional<int> { if (const char* e = getenv(name)) return atoi(e); return std::nullopt; };
    LdpcOverrides o;
    o.pr = get("DVBS2_PR"); o.pr_w1 = get("DVBS2_PR_W1"); o.pr_v2 = get("DVBS2_PR_V2"); o.dense = get("DVBS2_DENSE"); o.hz2 = get("DVBS2_HZ2");
    o.solo = get("DVBS2_SOLO"); o.soft_barrier = get("DVBS2_SOFT_BARRIER"); o.v2 = get("DVBS2_V2"); o.v2p = get("DVBS2_V2P");
    o.group_sync = get("DVBS2_GROUP_SYNC"); o.group_spin_max = get("DVBS2_GROUP_SPIN_MAX"); o.resolve_rounds = get("DVBS2_RESOLVE_ROUNDS");
    o.timing = getenv("DVBS2_TIMING") != nullptr;
    return o;
}

namespace {
bool pick(const std::optional<int>& o, bool rule) { return o ? *o != 0 : rule; } // the override where one is set, else the rule

// ---- which build of the sweep kernel (decided once, before the records are laid out for it) ----
struct Choice {
    std::string error;
    bool pr = false, pr_w1 = false, pr_v2 = false, dense = false, hz2 = false, solo = false, soft_bar = false;
    bool packed = false;  // the table's policy or forced; a pure-class table whose records do not fit still goes to the plain build (plan_ldpc)
    bool v2p_on = true;   // hazard layers with the packed first / last phase (classes v2p_class); DVBS2_V2P=0: tests
    bool pr_shared_sv = false;
    int dmax = 0, words_per_check = 0;
};
Choice select_build(const LdpcSchedule& s, const char* table_name, const LdpcOverrides& ov)
{
    Choice c;
    int degmax = 0, degmin = 1000;
    for (const LdpcLayer& L : s.layers) { degmax = std::max(degmax, L.cnt + 2); degmin = std::min(degmin, L.cnt + 2); }
    if (degmax > 32) { c.error = "check degree > 32 unsupported"; return c; }
    // "parity in records" variant (ldpc_kernel_pr.hpp): check degree <= 7, at most 4 hazard entries per layer, and two
    // pair workgroups must fit the 160 KB of LDS
    // Policy (measured on MI355X, tools/pr_sweep.sh; the two variants give identical bits): every eligible short and
    // medium table gains 12-43 % from the second workgroup per CU. On normal frames the classic kernel is as fast or
    // faster since its hazard layers run as lane chains (B4: 109 k vs 106 k frames/s; thin-layer tables lose up to
    // 20 % with parity-in-records).
    // Round 6: also the two NORMAL tables of check degree <= 4 (1/4 normal, S2X 2/9 normal: one-dword records, four frames per CU): interleaved A/B
    // 154.1 -> 158.9 k and 152.8 -> 157.6 k frames/s (+3.1 %); the other normal tables of degree <= 7 lose with it (2/5 0.958, B4 0.989, 1/3 0.941, S2X 13/45 0.849).
    c.pr = degmax <= 7 && pick(ov.pr, s.N < 64800 || degmax <= 4);
    for (const LdpcLayer& L : s.layers)
        if (L.block < 360 && (L.n_conflict > 4 || (L.n_conflict > 2 ? 4 : 2) > L.cnt)) c.pr = false;
    c.pr_shared_sv = 2 * pr_lds_bytes(s.N, s.K) > 160 * 1024; // (normal frames forced onto this kernel: one sign-vector area per workgroup)
    if (2 * pr_lds_bytes(s.N, s.K, c.pr_shared_sv) > 160 * 1024) c.pr = false;
    // degree class: the sweep kernel is built per multiple of four (message dwords per check); degree <= 4 tables that do not run the
    // parity-in-records kernel (1/4 normal, S2X 2/9 normal) get the one-dword class -- they move ~4.4 TB/s with two (+8 %)
    c.dmax = c.pr ? 8 : std::max(4, (degmax + 3) / 4 * 4);
    if (degmin < 3 || degmin <= c.dmax - 8) { c.error = "check degree spread unsupported by the kernel variants"; return c; }
    c.words_per_check = c.dmax / 4;
    // Short frames whose layers are mostly hazard layers (latency-bound ordered steps) and whose degree rules out the
    // parity-in-records kernel: the 80-VGPR build puts a second workgroup on the CU (measured: short 3/5 and 2/3 +34 %;
    // it costs 6-18 % where regular layers dominate, hence the 70 % threshold; degree classes above 12 do not fit 80 VGPRs).
    // It has no two-level lane chain (76 -> 349 spilled registers, round 3) and, since round 4, no single-pair lane chain either -- with
    // its tables addressed as LDS (typed pointers, ldpc_prims.hpp) the chain code made that build spill ten times as much (72 -> 725)
    // and short 3/5 / 2/3 lost 30 %; its layers take the block scheme.
    c.dense = !c.pr && c.dmax == 12 && 4 * half_lds_bytes(s.N) <= 160 * 1024 &&
              pick(ov.dense, s.N < 64800 && 10 * s.conflict_layers >= 7 * s.q);
    // Which of the other builds: measured per table (ldpc_policy.inc <- tools/policy_sweep.py + tools/gen_policy.py); a table
    // that is not listed takes the plain pair kernel.
    bool pol_packed = false, pol_solo = false;
    {
        struct Pol { const char* table; int packed, solo; };
        static const Pol kPolicy[] = {
#include "ldpc_policy.inc"
        };
        for (const Pol& p : kPolicy) if (!strcmp(p.table, table_name)) { pol_packed = p.packed; pol_solo = p.solo; }
    }
    // The build with the heavy-hazard paths (HZ2: up to twelve ordered entries per check instead of the one-wave walk, two-level walk
    // where one hazard pair is much closer than the rest): tables listed in ldpc_policy_hz2.inc (measured, tools/hz2_sweep.sh).
    bool pol_hz2 = false;
    {
        static const char* const kHz2[] = {
#include "ldpc_policy_hz2.inc"
        };
        for (const char* n : kHz2) if (!strcmp(n, table_name)) pol_hz2 = true;
    }
    c.hz2 = !c.dense && c.dmax >= 12 && pick(ov.hz2, pol_hz2);
    c.solo = !c.pr && !c.dense && !c.hz2 && c.dmax <= kSoloMaxDmax && !ov.timing && pick(ov.solo, pol_solo);
    // frame barriers in software (ldpc_prims.hpp, frame_barrier): by rule where no layer has hazards; with hazard layers only for the tables listed in
    // ldpc_policy_soft.inc (measured on two leases, tools/soft_sweep.py)
    bool pol_soft = s.conflict_layers == 0;
    {
        static const char* const kSoft[] = {
#include "ldpc_policy_soft.inc"
        };
        for (const char* n : kSoft) if (!strcmp(n, table_name)) pol_soft = true;
    }
    c.soft_bar = !c.pr && !c.dense && !c.solo && !c.hz2 && !ov.timing && c.dmax >= 20 && pick(ov.soft_barrier, pol_soft); // (built for the degree classes >= 20)
    c.packed = !c.pr && !c.dense && !c.hz2 && pick(ov.v2, pol_packed);
    c.v2p_on = pick(ov.v2p, true);
    // one-dword records (four 6-bit messages + the parity byte, ldpc_kernel_pr.hpp): check degree <= 4
    c.pr_w1 = c.pr && degmax <= 4 && pick(ov.pr_w1, true);
    if (c.pr_w1) c.words_per_check = 1;
    // packed nodes (check_node_v2_pr) in the regular middle layers of the two-dword-record kernel: per-wave sweep records as for the classic packed builds
    // Measured (MI355X, interleaved A/B x 3): short 2/5, 1/2, S2X short 26/45 / medium 1/3 +3.0 ... +3.8 %, short 1/3 +0.7 %; on NORMAL frames forced onto
    // this kernel (DVBS2_PR=1) B4 +2.1 % and S2X 9/20 +2.5 % on never-converging input -- and B4 9 % SLOWER at its operating point (Es/N0 2.0 dB: 353 -> 323 k frames/s;
    // this kernel's full syndrome test fetches the parity signs from the records): short / medium frames by rule, normal frames stay with the classic builds.
    c.pr_v2 = c.pr && !c.pr_w1 && pick(ov.pr_v2, s.N < 64800);
    return c;
}
LdpcBuild build_of(const Choice& c)
{
    if (c.pr) return c.pr_w1 ? LdpcBuild::pr_w1 : c.pr_v2 ? LdpcBuild::pr_packed : LdpcBuild::pr;
    if (c.dense) return LdpcBuild::dense;
    if (c.hz2) return LdpcBuild::hz2;
    if (c.soft_bar) return c.packed ? LdpcBuild::packed_soft : LdpcBuild::soft;
    if (c.solo) return c.packed ? LdpcBuild::packed_solo : LdpcBuild::solo;
    return c.packed ? LdpcBuild::packed : LdpcBuild::plain;
}

// ---- helpers of the record builders ----
const LdpcEntry& entry(const LdpcSchedule& s, const LdpcLayer& L, int k) { return s.entries[L.entry_off + k]; }

// The nearest pair (a, b) among the hazard entries of layer L (two entries of one group; distance d1 in rows) and the distance d2 of the
// next-nearest pair. The two-level walk (check_node_hazard) applies when the nearest pair is the layer's block and every other pair is at
// least twice as far apart -- the rows then go in outer blocks of d2 rows and only the near pair in ordered steps inside them.
struct NearPair { int a = -1, b = -1, d1 = 360, d2 = 360; bool two_level = false; };
NearPair nearest_pair(const LdpcSchedule& s, const LdpcLayer& L)
{
    NearPair p;
    for (int a = 0; a < L.n_conflict; a++)
        for (int b = a + 1; b < L.n_conflict; b++) {
            const LdpcEntry& ea = entry(s, L, a), & eb = entry(s, L, b);
            if (ea.base != eb.base) continue;
            const int d = std::abs((int)ea.rot - (int)eb.rot), dist = std::min(d, 360 - d);
            if (dist < p.d1) { p.d2 = p.d1; p.d1 = dist; p.a = a; p.b = b; }
            else p.d2 = std::min(p.d2, dist);
        }
    p.two_level = p.a >= 0 && p.d1 == L.block && p.d2 >= 2 * p.d1 && 360 / p.d1 - 360 / p.d2 >= 3;
    return p;
}

// Orientation of a chain pair: X's bit of row r is Y's bit of row r + block  <=>  (rotX - rotY) mod 360 == block.
// 0: (a, b) is (X, Y); 1: (b, a) is; -1: the two are no pair of one group at that distance.
int pair_orientation(const LdpcEntry& a, const LdpcEntry& b, int block)
{
    if (a.base != b.base) return -1;
    const int D = ((int)a.rot - (int)b.rot + 360) % 360;
    return D == block ? 0 : 360 - D == block ? 1 : -1;
}

// The entries order[k0 .. cnt) of layer L (order == null: schedule order) as wave w sees them: "mixed" = the wrap point 360 - rot lies
// inside the wave's rows, so some of its lanes read below it and some above; "plain" = one window offset serves the whole wave.
bool is_mixed(const LdpcEntry& e, int w) { const int thr = 360 - (int)e.rot; return 64 * w < thr && thr <= std::min(64 * w + 63, 359); }
struct WaveSplit { std::vector<int> mixed, plain; };
WaveSplit split_wave(const LdpcSchedule& s, const LdpcLayer& L, const int* order, int k0, int w)
{
    WaveSplit sp;
    for (int k = k0; k < L.cnt; k++) { const int e = order ? order[k] : k; (is_mixed(entry(s, L, e), w) ? sp.mixed : sp.plain).push_back(e); }
    return sp;
}

// ---- per-layer records ----
struct LayerRecords {
    std::vector<uint32_t> recs;
    std::vector<std::vector<int>> order; // record order of every layer's entries (ordered entries first, host-oriented pairs)
    std::vector<int> nc;                 // ordered entries the kernel handles in the layer's ordered phase (2, 4, 8, 12; kHazardWalk)
};
LayerRecords layer_records(const LdpcSchedule& s, const Choice& c)
{
    const int RS = rec_stride(c.dmax);
    LayerRecords lr{ std::vector<uint32_t>((size_t)s.q * RS, 0), std::vector<std::vector<int>>(s.q), std::vector<int>(s.q, 0) };
    for (int i = 0; i < s.q; i++) {
        const LdpcLayer& L = s.layers[i];
        uint32_t* rec = &lr.recs[(size_t)i * RS];
        uint32_t nc_code = 0;
        if (L.block < 360) {
            nc_code = L.n_conflict <= 2 ? 2 : L.n_conflict <= 4 ? 4 : L.n_conflict <= 8 ? 8 : 12;
            if (L.n_conflict > (c.hz2 && c.dmax <= kMaxHazard12Dmax ? kMaxHazardHz2 : kMaxHazard) || (int)nc_code > L.cnt) nc_code = kHazardWalk;
        }
        const bool chain_scratch = L.block <= kChainMaxBlock && (s.N / 360) * kSvWords >= lane_chain_words(L.block); // a lane chain's scratch fits the sign-vector area
        // A layer whose only hazard is ONE pair (two entries of one group) with a small block is walked as a lane
        // chain (check_node_hazard): the pair is ordered so that entry 0's bit of row j is entry 1's bit of row
        // j + block (pair_orientation); kRecChain. Needs lane_chain_words(block) of scratch per
        // frame in the sign-vector area. (Rounds 2-3, integer walk: gains up to block 64, flat to 128, slightly negative at 180; round 4,
        // float walk and packed chain: +0.2...1.6 % at 180.)
        std::vector<int>& order = lr.order[i];
        for (int k = 0; k < L.cnt + 2; k++) order.push_back(k);
        bool chain = false;
        if (!c.dense && chain_scratch && nc_code == 2 && L.n_conflict == 2 && (L.cnt + 2 <= kLaneChainMaxDeg || (c.packed && v2p_class(c.dmax)))) {
            const int o = pair_orientation(entry(s, L, 0), entry(s, L, 1), L.block);
            if (o == 1) std::swap(order[0], order[1]);
            chain = o >= 0;
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
        // two-level lane chain of check_node_hazard: the pair additionally has to be oriented like a single-pair chain, kRecChain;
        // not in the 80-VGPR build: the chain's state does not fit there, 76 -> 349 spilled registers)
        const bool tlc_build = tlc_class(c.dmax) && !c.hz2 && !c.pr && !c.dense && !c.soft_bar; // (kTlc<DMAX, HZ2> && !SOFT && MINW == 1 in the kernel)
        if (tlc_build && L.block < 360 && chain_scratch && (nc_code == 4 || nc_code == 8)) {
            NearPair p = nearest_pair(s, L);
            if (p.two_level) {
                if (pair_orientation(entry(s, L, p.a), entry(s, L, p.b), L.block) != 0) std::swap(p.a, p.b);
                chain = true;
                near_pair_first(p);
            }
        }
        if (c.hz2 && L.block < 360 && nc_code >= 4 && nc_code != (uint32_t)kHazardWalk && (L.cnt + 2 < 29 || nc_code == 8)) {
            const NearPair p = nearest_pair(s, L);
            if (p.two_level) near_pair_first(p);
        }
        lr.nc[i] = (int)nc_code;
        if (c.pr) chain = false; // that kernel has no lane chain (80 VGPRs)
        rec[0] = L.cnt | (nc_code << kRecNcShift) | (chain ? kRecChain : 0u) | ((uint32_t)L.sync_before << kRecSyncShift) | ((uint32_t)L.block << kRecBlockShift);
        rec[2] = block2;
        for (int k = 0; k < L.cnt + 2; k++) {
            const LdpcEntry& e = entry(s, L, order[k]);
            rec[4 + 2 * k] = (uint32_t)e.base + e.rot;
            rec[5 + 2 * k] = 360u - e.rot;
        }
    }
    if (c.pr) {
        const int q = s.q;
        lr.recs[(size_t)(q - 1) * RS + 4 + 2 * s.layers[q - 1].cnt] = (uint32_t)s.K;          // own parity of the last layer: row q-1 at offset K
        lr.recs[(size_t)(q - 1) * RS + 5 + 2 * s.layers[q - 1].cnt] = 360u;
        lr.recs[(size_t)0 * RS + 4 + 2 * (s.layers[0].cnt + 1)] = (uint32_t)s.K + 359u;     // previous parity of layer 0: same row, one lane down
        lr.recs[(size_t)0 * RS + 5 + 2 * (s.layers[0].cnt + 1)] = 1u;
    }
    return lr;
}

// ---- per-(layer, wave) records ----
// Sweep records per (layer, wave) for the classic kernel (check_node_v2 in ldpc_node_packed.hpp). A regular layer i > 0 gets,
// for each of the six waves of a frame, its data entries reordered "mixed first" (split_wave), window offsets pre-adjusted for the
// wave, and the lane masks of the mixed entries; a wave with more mixed entries than fix slots, layer 0 and hazard layers keep the
// classic record (replicated).
std::vector<uint32_t> wave_records(const LdpcSchedule& s, const Choice& c, const LayerRecords& lr)
{
    const int dmax = c.dmax, RS = rec_stride(dmax), RSW = rec_stride_wave(dmax);
    std::vector<uint32_t> wr((size_t)s.q * 6 * RSW, 0);
    for (int i = 0; i < s.q; i++) {
        const LdpcLayer& L = s.layers[i];
        const bool hazard = L.block < 360;
        // single-pair hazard layers walked by the packed register chain (check_node_chain_v2, built for the degree classes <= 16): block <=
        // kChainMaxBlock, the pair are the first two entries (schedule compiler), and on every wave the mixed regular entries fit the fix slots after the pair's
        int chain_order = -1;
        if (i > 0 && c.packed && dmax <= 16 && hazard && L.block <= kChainMaxBlock && L.n_conflict == 2 && L.cnt >= 2)
            chain_order = pair_orientation(entry(s, L, 0), entry(s, L, 1), L.block);
        for (int w = 0; chain_order >= 0 && w < 6; w++)
            if ((int)split_wave(s, L, nullptr, 2, w).mixed.size() > v2_nfix(dmax)) chain_order = -1;
        const bool chain2 = chain_order >= 0;
        // hazard layers of the packed builds whose ordered phase is the generic one (check_node_hazard with packed_phases, ldpc_node_hazard.hpp): the NC
        // ordered entries keep their record order in the first fix slots, the mixed regular entries follow; dmax / 2 fix slots in all
        const int ncv = lr.nc[i];
        const bool v2p = c.packed && c.v2p_on && v2p_class(dmax) && hazard && !chain2 && (ncv == 2 || ncv == 4 || ncv == 8) && (int)L.cnt >= ncv;
        // (parity-in-records: the last layer keeps its plain node, like layer 0; check_node_v2_pr exists for the degrees 5 .. 7)
        const bool packed_layer = i > 0 && (hazard ? chain2 || v2p : c.packed || (c.pr_v2 && i != s.q - 1 && L.cnt + 2 >= 5));
        for (int w = 0; w < 6; w++) {
            uint32_t* rec = &wr[((size_t)i * 6 + w) * RSW];
            std::copy(lr.recs.begin() + (size_t)i * RS, lr.recs.begin() + (size_t)(i + 1) * RS, rec);
            if (!packed_layer) continue;
            const WaveSplit sp = v2p ? split_wave(s, L, lr.order[i].data(), ncv, w) : split_wave(s, L, nullptr, chain2 ? 2 : 0, w);
            const int nfix = v2p ? std::min(dmax / 2, (int)L.cnt) - ncv : std::min(v2_nfix(dmax), (int)L.cnt);
            if (!chain2 && (int)sp.mixed.size() > nfix) continue; // (a chain layer was checked for every wave beforehand)
            std::fill(rec + 4, rec + RSW, 0u);
            rec[0] |= kRecPacked | (v2p ? kRecPackedHazard : 0u);
            const int lo = 64 * w;
            int slot = 0;
            auto put = [&](int k, bool mixed) {
                const LdpcEntry& e = entry(s, L, k);
                const int thr = 360 - (int)e.rot;
                const uint32_t S0 = (uint32_t)e.base + e.rot;
                uint32_t off = S0;                       // every row of the wave below the wrap point
                if (mixed || lo >= thr) off = S0 - 360u; // wrapped (mixed: the lanes below the wrap point get + 360 back)
                rec[4 + slot] = off;
                if (mixed) {
                    unsigned long long m = 0;
                    for (int l = 0; l < 64; l++) if (std::min(lo + l, 359) < thr) m |= 1ull << l; // threads 360..383 mirror row 359
                    rec[4 + dmax + 2 * slot] = (uint32_t)m; rec[4 + dmax + 2 * slot + 1] = (uint32_t)(m >> 32);
                }
                slot++;
            };
            auto put_ordered = [&](int k) { put(k, is_mixed(entry(s, L, k), w)); };
            if (chain2) { put_ordered(chain_order); put_ordered(1 - chain_order); } // the pair X, Y (the per-layer record already holds them in chain order) takes the first two fix slots
            if (v2p) for (int k = 0; k < ncv; k++) put_ordered(lr.order[i][k]);      // ordered entries, in the per-layer record's order
            for (int k : sp.mixed) put(k, true);
            for (int k : sp.plain) put(k, false);
            put(L.cnt, false);     // own parity (rot 0)
            put(L.cnt + 1, false); // previous parity (rot 0 for i > 0)
        }
    }
    return wr;
}

// "Pure" packed builds (ldpc_kernel.hpp, kPure: the packed builds of the degree class 32) have the plain nodes for layer 0 only: a
// (layer > 0, wave) record that is NOT in the packed format -- more mixed entries than fix slots, a one-wave walk layer -- would do no work
// there and the decode would be silently wrong. The test looks at the records that were actually BUILT. True: *layer, *wave name one.
bool has_unpacked_record(const LdpcSchedule& s, const std::vector<uint32_t>& wr, int RSW, int* layer, int* wave)
{
    for (int i = 1; i < s.q; i++)
        for (int w = 0; w < 6; w++) {
            const uint32_t h0 = wr[((size_t)i * 6 + w) * RSW];
            if (!(h0 & kRecPacked) || (s.layers[i].block < 360 && !(h0 & kRecPackedHazard))) { *layer = i; *wave = w; return true; }
        }
    return false;
}

// What the parity carry of the run loop relies on (check_node_v2 with RUN, ldpc_node_packed.hpp; the degree classes up to 8). The run
// loop takes EVERY packed regular record of a layer 0 < i < q - 1 (ldpc_kernel.hpp, kRun; a run may be that one trip), so each of them
// must have its own-parity slot 360 bytes behind its previous-parity slot and neither of the two a fix slot (a parity entry has no
// rotation): the trip reads own parity at offset 360 of the previous-parity address and writes it back through the own-parity slot.
// Where the next layer's record of the wave continues the run (same block, format and degree, and itself such a record), its
// previous-parity slot must name the byte of this record's own-parity slot: it takes that byte from the carry. The test looks at the
// records that were actually BUILT. False: *layer, *wave name the record (of a pair: the first) that breaks it.
bool parity_chain_ok(const LdpcSchedule& s, const std::vector<uint32_t>& wr, int dmax, int* layer, int* wave)
{
    const int RSW = rec_stride_wave(dmax);
    constexpr uint32_t kKey = (~0u << kRecBlockShift) | kRecPacked | 0xffu; // block, format and degree: the run loop's key
    auto mask = [&](const uint32_t* r, int slot) { return slot < v2_nfix(dmax) ? r[4 + dmax + 2 * slot] | r[4 + dmax + 2 * slot + 1] : 0u; };
    for (int i = 1; i + 1 < s.q; i++)
        for (int w = 0; w < 6; w++) {
            const uint32_t* a = &wr[((size_t)i * 6 + w) * RSW];
            const uint32_t* b = a + (size_t)6 * RSW;
            if (!(a[0] & kRecPacked) || (a[0] >> kRecBlockShift) < 360u) continue;
            const int own = (int)(a[0] & 0xffu), prev = own + 1; // slots behind the data entries
            bool ok = a[4 + own] == a[4 + prev] + 360u && !mask(a, own) && !mask(a, prev);
            if (i + 2 < s.q && (a[0] & kKey) == (b[0] & kKey)) ok = ok && b[4 + prev] == a[4 + own]; // (b is checked as a record in its own turn)
            if (!ok) { *layer = i; *wave = w; return false; }
        }
    return true;
}
} // namespace

LdpcPlan plan_ldpc(const LdpcSchedule& s, const char* table_name, int group_size, const LdpcOverrides& ov)
{
    LdpcPlan p;
    Choice c = select_build(s, table_name, ov);
    if (!c.error.empty()) { p.error = c.error; return p; }
    const LayerRecords lr = layer_records(s, c);
    p.wrecs = wave_records(s, c, lr);
    const int RSW = rec_stride_wave(c.dmax);
    int bad_layer = 0, bad_wave = 0;
    // A pure-class table that does not fit the packed format takes the plain build (of the 57 tables this concerns 9/10 normal only,
    // which fits); so does one whose hazard layers are kept off the packed phases (DVBS2_V2P=0), whatever its layers.
    if (c.packed && v2_pure_class(c.dmax) && (!c.v2p_on || has_unpacked_record(s, p.wrecs, RSW, &bad_layer, &bad_wave))) {
        c.packed = false;
        p.wrecs = wave_records(s, c, lr); // (the per-layer records stay as laid out for the packed build: chain bits of its single-pair layers included)
    }
    if (c.packed && v2_pure_class(c.dmax) && has_unpacked_record(s, p.wrecs, RSW, &bad_layer, &bad_wave)) { // the plan that is returned: refuse loudly
        p.error = "internal: a (layer, wave) record of a pure packed build is not in the packed format (layer " + std::to_string(bad_layer) + ", wave " + std::to_string(bad_wave) + ")";
        return p;
    }
    if (c.packed && !c.pr && c.dmax <= 8 && !parity_chain_ok(s, p.wrecs, c.dmax, &bad_layer, &bad_wave)) { // (the run loop's classes: ldpc_kernel.hpp, kRun)
        p.error = "internal: the parity slots of a packed regular record do not fit the run loop's parity carry (layer " + std::to_string(bad_layer) + ", wave " + std::to_string(bad_wave) + ")";
        return p;
    }
    p.recs = lr.recs;
    p.build = build_of(c);
    p.pr = c.pr; p.pr_shared_sv = c.pr_shared_sv; p.dmax = c.dmax; p.words_per_check = c.words_per_check;
    // Group-synchronous stop (ldpc_prims.hpp, group_decide): the frames of a group agree after every syndrome test, so the whole
    // group stops at the reference's count inside the first pass and the resolution rounds have nothing left to do (they stay as
    // the fallback; with the rule on, none is enqueued ahead of time). Needs the members of a group resident together: groups of up
    // to 64 frames (at most 32 pair workgroups of 256 CUs). DVBS2_GROUP_SYNC=0 / 1 overrides (tests run both).
    p.gsync_on = group_size <= 64 && pick(ov.group_sync, true);
    if (p.gsync_on) p.resolve_rounds = 0;
    if (ov.group_spin_max) p.spin_max = std::max(0, *ov.group_spin_max);                          // tests: 0 = a waiting member gives up at once (fallback path)
    if (ov.resolve_rounds) p.resolve_rounds = std::max(0, std::min(8, *ov.resolve_rounds)); // tests: 0 forces the host-side leftover path
    static const char* const kSuffix[kLdpcBuilds] = { ">", ", packed>", ", solo>", ", packed, solo>", ", hz2>", ", soft>", ", packed, soft>", ", dense>",
                                                      "", "<w1>", "<packed>" };
    p.kernel_name = std::string(c.pr ? "ldpc_layered_pr_kernel" : "ldpc_layered_kernel<" + std::to_string(c.dmax)) + kSuffix[(int)p.build];
    p.solo_lds_bytes = half_lds_bytes(s.N);
    p.lds_bytes = c.pr ? pr_lds_bytes(s.N, s.K, c.pr_shared_sv) : 2 * p.solo_lds_bytes;
    return p;
}

} // namespace dvbs2
