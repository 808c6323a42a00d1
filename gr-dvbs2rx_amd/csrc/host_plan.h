// host_plan.h -- how a host-buffer call (dvbs2_ldpc_decode, dvbs2_chain_decode, dvbs2_chain_decode_llr) is cut into chunks. Plain C++,
// no HIP: tests/test_host_plan.py compiles it with the host compiler.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace dvbs2 {

// Plan of a call of n_frames frames, as (first frame, frames) chunks of whole LDPC groups of G frames (an even number of frames: two
// frames per workgroup); chunk c uses slot and stream c % kSlots, so that transfers and decodes of neighbouring chunks overlap.
// in_locked: the caller's input buffer is page-locked; in_symbols: it holds XFECFRAME symbols (8 bytes each), not int8 LLRs;
// host_chunk (DVBS2_HOST_CHUNK; 0: unset) and host_plan (DVBS2_HOST_PLAN; empty: unset) are the experiment / test knobs.
//
// The decode of a chunk starts when its input has arrived and a launch of up to 512 frames (one frame pair per CU) takes as long as a
// smaller one, so the FIRST chunk is 512 frames; every further chunk boundary costs a launch gap that the single resident launch does
// not have. Pageable input: the runtime stages the copy through its own pinned buffer while the calling thread waits, so the copy of
// chunk c + 1 has to run under the decode of chunk c: chunks of 1024. Page-locked input (dvbs2_host_register / hipHostMalloc): the link
// moves 57 GB/s (bench.py host_link), the whole input of 4096 normal frames arrives in under 5 ms through the copy stream: one large
// middle chunk, and a small last one so that little output is left to fetch when the decode ends.
inline std::vector<std::pair<int, int>> host_chunk_plan(int n_frames, int G, bool in_locked, bool in_symbols, int host_chunk,
                                                        const std::string& host_plan)
{
    const int unit = G % 2 ? 2 * G : G;
    auto round_unit = [&](int x) { return std::max(unit, (x + unit - 1) / unit * unit); };
    std::vector<std::pair<int, int>> plan;
    if (!host_plan.empty()) { // experiments: comma list of chunk sizes, the last one repeats
        int f0 = 0, last = 512;
        for (const char* q = host_plan.c_str(); f0 < n_frames;) {
            if (*q) { last = std::max(2, atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
            const int nf = std::min(round_unit(last), n_frames - f0);
            plan.push_back({ f0, nf }); f0 += nf;
        }
    } else if (in_symbols && in_locked && !host_chunk) {
        // SYMBOL input is 8 bytes per symbol (172.8 KB per 8PSK normal frame, 2.7 x the LLR bytes): at a receiver's operating point the copy of a
        // chunk takes longer than its kernels, so page-locked input goes in uniform chunks of 512 frames (one launch wave of the GPU) -- the copy of
        // chunk c + 1 runs under the kernels of chunk c and the call ends one chunk's kernels after its last byte arrived. Measured (MI355X, 4096
        // frames of 8PSK 3/4 normal, page-locked buffers): 512 | 3072 | 512 (the plan for LLR input) 221 k frames/s at Es/N0 8.5 dB = 0.67 of the link
        // bound -- the GPU idles while 531 MB arrive -- and 0.853 of the resident rate on never-converging input; uniform 512: 291 k (0.88 of the
        // link bound) and 0.899. Chunks of 128 for 512-frame calls LOSE (a launch of 128 frames takes as long as one of 512): 181 -> 144 k.
        const int chunk = round_unit(512);
        for (int f0 = 0; f0 < n_frames; f0 += chunk) plan.push_back({ f0, std::min(chunk, n_frames - f0) });
    } else if (in_locked && n_frames > 1024 && !host_chunk) {
        // measured (MI355X, 4096 frames of table B4, tools/host_entry_ab.py): 512 | 3072 | 512 -> 97.3 % of the resident rate, 512 | 3584
        // 97.3 %, 512 | 1536 | 1536 | 512 96.7 %, eight chunks of 512 93.6 %, four of 1024 95.0 %
        // every boundary is a multiple of `unit` (frame_base of enqueue()) and none lies past the call's last frame (a group size above
        // 512 -- or an odd one above 256 -- makes `unit` larger than the first chunk: ADVICE r4)
        const int b1 = std::min(round_unit(512), n_frames);
        const int b2 = std::min(std::max(b1, (n_frames - 512) / unit * unit), n_frames);
        const int bounds[4] = { 0, b1, b2, n_frames };
        for (int k = 0; k < 3; k++) if (bounds[k + 1] > bounds[k]) plan.push_back({ bounds[k], bounds[k + 1] - bounds[k] });
    } else {
        // pageable input (measured as above): 512, then chunks of 1024 -> 96.0-96.5 %; eight equal chunks of 512 95.0-95.4 %
        int first = 512, chunk = std::max(1024, (n_frames + 7) / 8);
        if (host_chunk) first = chunk = host_chunk; // experiments, tests
        first = round_unit(first); chunk = round_unit(chunk);
        for (int f0 = 0; f0 < n_frames;) { const int nf = std::min(f0 ? chunk : first, n_frames - f0); plan.push_back({ f0, nf }); f0 += nf; }
    }
    return plan;
}

} // namespace dvbs2
