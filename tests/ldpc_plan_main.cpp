// The LDPC planner (csrc/ldpc_plan.cpp) on the CPU. stdin: one row per line, "TABLE GROUP_SIZE [DVBS2_NAME=VALUE ...]" (the overrides go
// through the environment, like in a handle). stdout per row: "E <error text>\n", or
// "P kernel name|dmax|words_per_check|pr_shared_sv|lds_bytes|gsync_on|n_recs|n_wrecs|<first broken format invariant, empty: none>\n"
// followed by the raw words of recs and wrecs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include "../gr-dvbs2rx_amd/csrc/ldpc_plan.h"

using namespace dvbs2;

// What the kernels rely on in the records (the comments of ldpc_plan.cpp / ldpc_layout.h as checks). Empty: all hold.
static std::string check_format(const LdpcSchedule& s, const LdpcPlan& p)
{
    const int RS = rec_stride(p.dmax), RSW = rec_stride_wave(p.dmax), sv_words = (s.N / 360) * kSvWords;
    const bool packed_build = p.build == LdpcBuild::packed || p.build == LdpcBuild::packed_solo || p.build == LdpcBuild::packed_soft;
    auto at = [](int i, int w) { return " (layer " + std::to_string(i) + ", wave " + std::to_string(w) + ")"; };
    if ((int)p.recs.size() != s.q * RS || (int)p.wrecs.size() != s.q * 6 * RSW) return "record array sizes";
    for (int i = 0; i < s.q; i++) {
        const LdpcLayer& L = s.layers[i];
        const bool hazard = L.block < 360;
        for (int w = -1; w < 6; w++) { // -1: the per-layer record
            const uint32_t* rec = w < 0 ? &p.recs[(size_t)i * RS] : &p.wrecs[((size_t)i * 6 + w) * RSW];
            const uint32_t h0 = rec[0];
            if ((h0 & 0xff) != L.cnt || (h0 >> kRecBlockShift) != L.block) return "cnt / block of word 0" + at(i, w);
            if ((h0 & kRecChain) && p.pr) return "chain bit in a parity-in-records plan" + at(i, w);
            if ((h0 & kRecChain) && (!hazard || lane_chain_words(L.block) > sv_words)) return "chain bit, but the chain's scratch does not fit the sign-vector area" + at(i, w);
            if (w < 0) { if (h0 & (kRecPacked | kRecPackedHazard)) return "packed bits in a per-layer record" + at(i, w); continue; }
            if (i > 0 && packed_build && v2_pure_class(p.dmax) && (!(h0 & kRecPacked) || (hazard && !(h0 & kRecPackedHazard))))
                return "pure packed build: record not in the packed format" + at(i, w);
            if ((h0 & kRecPackedHazard) && !((h0 & kRecPacked) && hazard)) return "packed-hazard bit without packed bit / hazard layer" + at(i, w);
            if (!(h0 & kRecPacked)) continue;
            if (i == 0) return "packed record in layer 0" + at(i, w);
            // fix slots of the record kind: hazard layer with packed phases dmax / 2 in all; packed chain: the pair + v2_nfix; regular: v2_nfix
            const int nfix = (h0 & kRecPackedHazard) ? std::min(p.dmax / 2, (int)L.cnt) : hazard ? 2 + v2_nfix(p.dmax) : std::min(v2_nfix(p.dmax), (int)L.cnt);
            const int nslots = (RSW - 4 - p.dmax) / 2, lo = 64 * w;
            for (int slot = 0; slot < nslots; slot++) {
                const unsigned long long m = rec[4 + p.dmax + 2 * slot] | (unsigned long long)rec[4 + p.dmax + 2 * slot + 1] << 32;
                if (!m) continue;
                if (slot >= nfix) return "lane mask beyond the fix slots" + at(i, w);
                const uint32_t S0 = rec[4 + slot] + 360u; // a mixed entry's offset is S0 - 360
                int thr = -1;
                for (int k = 0; k < L.cnt; k++) { const LdpcEntry& e = s.entries[L.entry_off + k]; if ((uint32_t)e.base + e.rot == S0) thr = 360 - (int)e.rot; }
                if (thr < 0) return "masked slot is no data entry of the layer" + at(i, w);
                unsigned long long want = 0;
                for (int l = 0; l < 64; l++) if (std::min(lo + l, 359) < thr) want |= 1ull << l; // threads 360..383 mirror row 359
                if (m != want) return "lane mask is not the lanes below the wrap point" + at(i, w);
            }
        }
    }
    return "";
}

int main()
{
    static const char* const kNames[] = { "DVBS2_PR", "DVBS2_PR_W1", "DVBS2_PR_V2", "DVBS2_DENSE", "DVBS2_HZ2", "DVBS2_SOLO", "DVBS2_SOFT_BARRIER", "DVBS2_V2", "DVBS2_V2P",
                                          "DVBS2_GROUP_SYNC", "DVBS2_GROUP_SPIN_MAX", "DVBS2_RESOLVE_ROUNDS", "DVBS2_TIMING" };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string table, kv;
        int G = 0;
        in >> table >> G;
        for (const char* n : kNames) unsetenv(n);
        while (in >> kv) { const size_t eq = kv.find('='); setenv(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str(), 1); }
        LdpcSchedule s;
        LdpcPlan p;
        if (!compile_ldpc_schedule(find_ldpc_table(table.c_str()), &s)) p.error = "unknown or inconsistent LDPC table";
        else p = plan_ldpc(s, table.c_str(), G, LdpcOverrides::from_env());
        if (!p.error.empty()) { std::printf("E %s\n", p.error.c_str()); continue; }
        std::printf("P %s|%d|%d|%d|%zu|%d|%zu|%zu|%s\n", p.kernel_name.c_str(), p.dmax, p.words_per_check, (int)p.pr_shared_sv, p.lds_bytes, (int)p.gsync_on,
                    p.recs.size(), p.wrecs.size(), check_format(s, p).c_str());
        std::fwrite(p.recs.data(), 4, p.recs.size(), stdout);
        std::fwrite(p.wrecs.data(), 4, p.wrecs.size(), stdout);
    }
    return 0;
}
