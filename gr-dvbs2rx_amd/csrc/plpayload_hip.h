// plpayload_hip.h -- PLFRAME payload step on the device: PL descrambling, pilot removal and the
// per-segment phase de-rotation that plsync_cc_impl::handle_payload() applies before the symbols reach
// xfecframe_demapper_cb (reference lib/plsync_cc_impl.cc:644-653, :727-795; lib/pl_descrambler.cc).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "device_stage.h"
#include "pl_signal.h"

namespace dvbs2 {

class PlPayloadHip : public DeviceStage {
public:
    PlPayloadHip(int gold_code, int n_slots, int has_pilots, int max_frames, int device);
    int n_slots() const { return n_slots_; }
    int n_pilots() const { return n_pilots_; }
    int payload_len() const { return n_slots_ * 90 + n_pilots_ * 36; }
    int xfecframe_len() const { return n_slots_ * 90; }
    int max_frames() const { return max_frames_; }
    // DEVICE pointers. d_payload: n_frames * payload_len complex (re, im); per frame: PLHEADER phase, phase increment
    // per symbol (2 pi fine_foffset, 0 when the frame is not coarse-corrected), coarse-corrected flag, n_pilots pilot
    // phases (ignored without pilots / when not coarse-corrected); d_out: n_frames * xfecframe_len complex.
    int process_device(const float* d_payload, int n_frames, const float* d_plheader_phase, const float* d_phase_inc,
                       const int32_t* d_coarse_corrected, const float* d_pilot_phase, float* d_out, hipStream_t stream);
    // the same with frame f's payload at d_in + f * frame_stride + in_offset (complex symbols): whole PLFRAMEs (plframe_hip.h)
    int process_device_strided(const float* d_in, int frame_stride, int in_offset, int n_frames, const float* d_plheader_phase,
                               const float* d_phase_inc, const int32_t* d_coarse_corrected, const float* d_pilot_phase, float* d_out,
                               hipStream_t stream);
    const uint8_t* d_rn() const { return d_rn_; } // Rn(i), i < payload_len, on the device

private:
    int n_slots_, n_pilots_, has_pilots_, max_frames_;
    uint8_t* d_rn_ = nullptr;
};

} // namespace dvbs2
