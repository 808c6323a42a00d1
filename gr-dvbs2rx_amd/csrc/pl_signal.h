// pl_signal.h -- physical-layer signalling on the host: the PLHEADER and PLS rules every PL stage (plpayload, plframe, plsync, plcoarse,
// plframer) goes by. Plain C++, no HIP header: a host compiler alone builds pl_signal.cpp, and a test program links it without a kernel
// unit. The constexpr functions are also what the kernels call (a constexpr function needs no attribute in device code), so each rule
// is written once: frame shape from a PLSC, PLFRAME length from slots and pilot blocks, bit k of a PLHEADER.
#pragma once
#include <cstdint>
#include <string>

namespace dvbs2 {

constexpr uint32_t kSofWord = 0x18D2E82u;                  // 26 bits, first transmitted bit is bit 25 (lib/pl_defs.h:42)
constexpr uint64_t kPlscScrambler = 0x719d83c953422dfaull; // lib/pl_defs.h:44

// pilot blocks of a frame of n_slots slots (lib/pl_signaling.cc:51) and the PLFRAME length in symbols: header, slots, pilot blocks
constexpr int pl_pilot_blocks(int n_slots, int has_pilots) { return has_pilots ? ((n_slots - 1) >> 4) : 0; }
constexpr int pl_frame_len(int n_slots, int n_pilots) { return (n_slots + 1) * 90 + 36 * n_pilots; }

// Slots, pilot blocks and PLFRAME length of a PLSC: pls_info_t::parse (lib/pl_signaling.cc:19-61). A dummy frame has no pilots, and the
// reserved MODCODs 29..31 take the dummy frame's 36 slots WITH the short and pilot bits (the frame tracker relies on that).
struct PlFrameShape { int n_slots, n_pilots, plframe_len; };
constexpr PlFrameShape pl_frame_shape(int plsc)
{
    const int modcod = plsc >> 2, dummy = modcod == 0;
    int n_slots = modcod >= 1 && modcod <= 11 ? 360 : modcod >= 12 && modcod <= 17 ? 240 : modcod >= 18 && modcod <= 23 ? 180 :
                  modcod >= 24 && modcod <= 28 ? 144 : 36;
    if ((plsc & 2) && !dummy) n_slots >>= 2;
    const int n_pilots = pl_pilot_blocks(n_slots, (plsc & 1) && !dummy);
    return { n_slots, n_pilots, pl_frame_len(n_slots, n_pilots) };
}

// bit k (0 <= k < 90) of the PLHEADER whose scrambled PLSC codeword is cw (plsc_codeword(plsc) ^ kPlscScrambler): the SOF, then the
// codeword from its bit 63 down. PLSC 0 has the all-zero codeword, so its header is plheader_bit(kPlscScrambler, k).
constexpr int plheader_bit(uint64_t cw, int k) { return k < 26 ? (int)((kSofWord >> (25 - k)) & 1) : (int)((cw >> (89 - k)) & 1); }

// pls_info_t::parse (lib/pl_signaling.cc:19-61)
struct PlsInfo {
    int plsc, modcod, short_fecframe, has_pilots, dummy_frame, n_mod, n_slots, n_pilots, plframe_len, payload_len, xfecframe_len;
};
PlsInfo pls_parse(int plsc);
// the interleaved (64,7) Reed-Muller codeword of a PLSC, first transmitted bit in bit 63 (lib/reed_muller.cc:57-96)
uint64_t plsc_codeword(int plsc);
// the 90 expected PLHEADER symbols (re, im): SOF + scrambled PLSC codeword, pi/2-BPSK (lib/pi2_bpsk.cc:18-43)
void plheader_symbols(int plsc, float* syms90);
// rank[c] = position of codeword c in the enabled list (n = 0: all 128, in order), 255 = disabled; a repeated entry never
// wins over its first occurrence. Returns false for an index >= 128 (lib/reed_muller.cc:48-52)
bool pls_rank_table(const uint8_t* list, int n, uint8_t rank[128]);

// Rn(i) in 0..3, i < n, from the definition in ETSI EN 302 307-1 clause 5.5.4: x(i+18) = x(i+7) + x(i), x(0) = 1;
// y(i+18) = y(i+10) + y(i+7) + y(i+5) + y(i), y(0..17) = 1; z_n(i) = x((i + n) mod (2^18 - 1)) + y(i);
// Rn(i) = 2 z_n((i + 131072) mod (2^18 - 1)) + z_n(i). (The reference reaches the same numbers with register masks.)
void pl_scrambling_rn(int gold_code, uint8_t* rn, int n);

// the tap signs of the frame search (plsync_hip.h: plsync_tap_bits) at run time from the 90 expected symbols of PLSC 0: imaginary parts
// (+-1) of the 25 SOF taps (header positions 1..25) and the 32 PLSC taps (positions 27, 29 .. 89)
void plsync_taps(float* sof25, float* plsc32);

// the weighting window of lib/pl_freq_sync.cc:74-85 as the floats the reference keeps: 89 values (full) or 25 (SOF)
int plcoarse_weights(int full, float* w);

// what the framer kernel reads per frame; offsets in complex symbols, all even (every frame length, 90, 1440 and 1476 is even)
struct PlFramerRec {
    int64_t in_offset;  // of the frame's XFECFRAME in the input (a dummy frame consumes none: the offset of the next data frame)
    int64_t out_offset; // of the frame's PLFRAME in the output
    int32_t n_slots, n_pilots;
    int32_t plsc, dummy;
};
static_assert(sizeof(PlFramerRec) == 32, "the record is read as two 16-byte halves");

// The verdict on one PLSC: nullptr, or why dvbs2_plframe_create would refuse it.
const char* plframer_refusal(int plsc);
// The records of a sequence, rec[n_frames] (nullable), and the two totals (nullable). false: *err says which frame and why.
// The one place where the offsets are formed: dvbs2_plframer_layout and PlFramerHip::set_sequence both call it.
bool plframer_layout(const uint8_t* plsc, int n_frames, PlFramerRec* rec, int64_t* in_syms, int64_t* out_syms, std::string* err);

} // namespace dvbs2
