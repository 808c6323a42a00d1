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
#include "pl_signal.h" // PlFramerRec, plframer_layout, plheader_symbols, pl_scrambling_rn

namespace dvbs2 {

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
    // 90 PLHEADER symbols of that PLSC. Writes exactly out_offset[n_frames] (+ 90) symbols. The entry (c_api_plframer.hip) checks the arguments.
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
