// bbframer_hip.h -- BB framing on the device: mode adaptation for MPEG-TS (EN 302 307-1 clauses 5.1.4 to 5.1.6), the mirror of
// bbdeheader_hip.h. 188-byte TS packets in, BBFRAMEs of kbch / 8 bytes out: BBHEADER (MATYPE, UPL, DFL, SYNC, SYNCD, CRC-8), a
// DATAFIELD cut from the CRC-encoded packet stream E, zero padding. In the reference's transmit flowgraph the place is held by gr-dtv's
// dvb_bbheader_bb (apps/dvbs2-tx:619-621). notes/bbframer.md has the definitions.
//   E[188 p + i] = P[p][i] for i = 1..187;  E[188 p] = CRC-8 of P[p - 1][1..187] for p >= 1;  E[0] = P[0][0]
// A handle holds pos, the bytes of E consumed since create / reset. pos is arithmetic on the call arguments and is mirrored on the
// host; what travels between calls on the device is the last packet presented (its unconsumed tail is the head of the next call's
// first DATAFIELD) and its finished CRC.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include "device_stage.h"

namespace dvbs2 {

constexpr int kBbfHeaderBytes = 10; // BBHEADER
constexpr int kBbfTsLen = 188;      // UPL / 8

// ---- host only, no device
// the check byte of `data`: remainder of data * x^8 modulo x^8 + x^7 + x^6 + x^4 + x^2 + 1, zero start, no reflection
int crc8(const uint8_t* data, size_t n);
// ten BBHEADER bytes with their CRC-8; -1: a field does not fit (matype1, matype2, sync in 0..255, the three lengths in 0..65535)
int bbheader_build(uint8_t out[10], int matype1, int matype2, int upl_bits, int dfl_bits, int sync, int syncd_bits);
// packets the call (n_frames, dfl_bytes) reads at position pos: ceil((pos + n_frames * dfl_bytes) / 188) - ceil(pos / 188); dfl_bytes > 0
int64_t bbframer_need(uint64_t pos, int n_frames, int dfl_bytes);
// the arguments of a create: empty, or the text of the refusal (kArgument)
std::string bbframer_check_create(int kbch_bits, int max_frames);
// the arguments of a call on a handle (max_frames, max_dfl_bytes): 0, or kArgument / kSize with the text in *text
int bbframer_check_call(int max_frames, int max_dfl_bytes, int n_frames, int dfl_bytes, std::string* text);

struct BbfState { // what a call leaves for the next one
    unsigned long long packets, bbframes;
    unsigned char last_crc;            // finished CRC of the last packet presented
    unsigned char last_pkt[kBbfTsLen]; // the last packet presented; its tail from pos % 188 on is not consumed yet
};
struct BbfDevice { // device-resident (one per handle): a call reads one copy of the state and writes the other, the host alternates
    BbfState st[2];
    unsigned long long sync_errors; // only ever added to atomically
};
struct BbfCounters { unsigned long long packets, bbframes, sync_errors; };

class BbFramerHip : public DeviceStage {
public:
    BbFramerHip(int kbch_bits, int max_frames, int device);
    int kbch_bytes() const { return kbch_bytes_; }
    int max_dfl_bytes() const { return kbch_bytes_ - kBbfHeaderBytes; }
    int max_frames() const { return max_frames_; }
    int max_packets_per_call() const { return (int)(((int64_t)max_frames_ * max_dfl_bytes() + kBbfTsLen - 1) / kBbfTsLen); }
    uint64_t pos() const { return pos_; }
    int set_matype(int matype1, int matype2); // later calls
    // host only: packets the NEXT call (n_frames, dfl_bytes) reads; -1 with the call's error for refused arguments
    int need(int n_frames, int dfl_bytes, int* n_packets);
    // DEVICE pointers: need() whole packets at d_ts -> n_frames BBFRAMEs of kbch_bytes back to back at d_bbframes. Asynchronous on
    // `stream`, no allocation, no synchronisation, one launch. The two ranges must not overlap.
    int process_device(const uint8_t* d_ts, int n_frames, int dfl_bytes, uint8_t* d_bbframes, hipStream_t stream);
    int counters(BbfCounters* out, hipStream_t stream); // synchronises `stream`
    int reset(hipStream_t stream);                // pos 0, nothing carried, counters zero

private:
    int kbch_bytes_, max_frames_;
    int matype1_ = 0xF2, matype2_ = 0;
    int crc_serial_ = 0; // measurement only: one lane per CRC (notes/bbframer.md)
    uint64_t pos_ = 0;   // host mirror, advanced when a call was launched
    int cur_ = 0;        // the copy of the state the next call reads
    BbfDevice* d_ = nullptr;
};

} // namespace dvbs2
