// plframer_hip.h -- PL framing on the device, the last step of the forward direction (enc_hip.h gives the XFECFRAMEs): PLHEADER,
// pilot blocks and PL scrambling of a SEQUENCE of frames with mixed MODCODs and dummy frames (ETSI EN 302 307-1 clauses 5.5.1 - 5.5.4;
// dvbs2_physical_cc in the reference's transmit flowgraph, apps/dvbs2-tx:619-636, is gr-dtv's and not part of the reference tree).
// It is the exact inverse of pl_payload_kernel (plpayload_hip.hip) with zero phases: multiplying by j^Rn is a swap and a sign flip,
// PLHEADER symbols and pilots are constants, so every output is defined bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "device_stage.h"
#include "plframe_hip.h" // pls_parse, plheader_symbols, pl_scrambling_rn

namespace dvbs2 {

// what the kernel reads per frame; offsets in complex symbols, all even (every frame length, 90, 1440 and 1476 is even)
struct PlFramerRec {
    int64_t in_offset;  // of the frame's XFECFRAME in the input (a dummy frame consumes none: the offset of the next data frame)
    int64_t out_offset; // of the frame's PLFRAME in the output
    int32_t n_slots, n_pilots;
    int32_t plsc, dummy;
};
static_assert(sizeof(PlFramerRec) == 32, "the record is read as two 16-byte halves");

// Host only. The verdict on one PLSC: nullptr, or why dvbs2_plframe_create would refuse it.
inline const char* plframer_refusal(int plsc)
{
    if (plsc < 0 || plsc > 127) return "out of range (0..127)";
    const PlsInfo p = pls_parse(plsc);
    return p.n_mod == 0 && !p.dummy_frame ? "names a reserved MODCOD (29..31)" : nullptr;
}

// Host only: the records of a sequence, rec[n_frames] (nullable), and the two totals (nullable). false: *err says which frame and why.
// The one place where the offsets are formed: dvbs2_plframer_layout and PlFramerHip::set_sequence both call it.
inline bool plframer_layout(const uint8_t* plsc, int n_frames, PlFramerRec* rec, int64_t* in_syms, int64_t* out_syms, std::string* err)
{
    int64_t in = 0, out = 0;
    for (int f = 0; f < n_frames; f++) {
        if (const char* why = plframer_refusal(plsc[f])) {
            if (err) *err = "plsc[" + std::to_string(f) + "] " + why;
            return false;
        }
        const PlsInfo p = pls_parse(plsc[f]);
        if (rec) rec[f] = { in, out, p.n_slots, p.n_pilots, p.plsc, p.dummy_frame };
        in += p.dummy_frame ? 0 : p.xfecframe_len;
        out += p.plframe_len;
    }
    if (in_syms) *in_syms = in;
    if (out_syms) *out_syms = out;
    return true;
}

class PlFramerHip : public DeviceStage {
public:
    PlFramerHip(int gold_code, int max_frames, int device);
    int max_frames() const { return max_frames_; }
    int n_frames() const { return (int)rec_.size(); } // of the sequence; a fresh handle has none
    int64_t in_syms() const { return in_syms_; }
    int64_t out_syms() const { return out_syms_; }
    // symbols the first n frames of the sequence read and write (n <= n_frames()); in_end == 0: dummy frames only, no input is read
    int64_t in_end(int n) const { return n < n_frames() ? rec_[n].in_offset : in_syms_; }
    int64_t out_end(int n) const { return n < n_frames() ? rec_[n].out_offset : out_syms_; }
    // Configuration call, synchronous (one hipMemcpy): not while work of the handle is in flight. n_frames 0..max_frames.
    int set_sequence(const uint8_t* plsc, int n_frames);
    // DEVICE pointers, one launch, asynchronous on `stream`. Frames the first n_frames of the sequence; closing_plsc >= 0 appends the
    // 90 PLHEADER symbols of that PLSC. Writes exactly out_offset[n_frames] (+ 90) symbols. The entry (c_api_pl.hip) checks the arguments.
    int frame_device(const float* d_xfecframes, int n_frames, int closing_plsc, float* d_plframes, hipStream_t stream);

private:
    int max_frames_;
    std::vector<PlFramerRec> rec_;
    std::vector<int> longest_; // longest_[f]: the longest plframe_len among frames 0..f (grid.x of a call that frames f + 1 of them)
    int64_t in_syms_ = 0, out_syms_ = 0;
    uint8_t* d_rn_ = nullptr;      // Rn(k), k < 33192: the longest payload
    float* d_hdr_ = nullptr;       // 128 x 90 PLHEADER symbols (re, im); the reserved MODCODs' rows are there and never read
    PlFramerRec* d_rec_ = nullptr; // max_frames records
};

} // namespace dvbs2
