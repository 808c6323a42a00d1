// plframe_hip.h -- PLFRAME front end on the device: everything that PRODUCES the per-frame parameters
// of the payload step once frame boundaries are known -- PLSC decoding of the frame's own header (reference
// lib/plsync_cc_impl.cc:582-590, lib/pl_signaling.cc:114-167, lib/reed_muller.cc:120-210, lib/pi2_bpsk.cc:45-196), the
// data-aided phases of SOF / PLHEADER / pilot blocks (lib/pl_freq_sync.cc:201-273) and the fine frequency offset
// (:275-349) -- followed by the payload step itself (plpayload_hip.h) reading whole PLFRAMEs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "device_stage.h"
#include "plpayload_hip.h"
#include "pl_signal.h"

namespace dvbs2 {

// What the two stages that decode PLSCs on the device (PlFrameHip, PlSyncHip) have in common: the decoder's mode and the
// enabled-codeword list of the reference's second plsc_decoder constructor, in the caller's order (n = 0: all 128).
class PlscListStage : public DeviceStage {
public:
    void set_plsc_mode(int coherent, int soft) { coherent_ = coherent ? 1 : 0; soft_ = soft ? 1 : 0; }
    int set_expected_pls(const uint8_t* list, int n);

protected:
    using DeviceStage::DeviceStage;
    int coherent_ = 1, soft_ = 1;
    uint8_t* d_rank_ = nullptr; // 128 bytes: position of each codeword in the enabled list, 255 = disabled
};

// device (or host-staged) outputs of the estimate kernel, each nullable
struct PlFrameEstimates {
    uint8_t* plsc_decoded = nullptr;
    float* sof_phase = nullptr;
    float* plheader_phase = nullptr;
    float* pilot_phase = nullptr;
    float* fine_foffset = nullptr;
    int32_t* fine_valid = nullptr;
};

class PlFrameHip : public PlscListStage {
public:
    // plsc is checked by dvbs2_plframe_create, which alone constructs this: within 0..127 and no reserved MODCOD
    PlFrameHip(int gold_code, int plsc, int max_frames, int device);
    ~PlFrameHip();
    const PlsInfo& pls() const { return pls_; }
    int max_frames() const { return max_frames_; }
    // DEVICE pointers. d_plframes: n_frames * plframe_len complex (+ 90 when has_trailing_header); d_coarse_corrected:
    // n_frames int32; d_coarse_foffset: n_frames float, needed only by pilotless handles. d_out (nullable = estimates
    // only): n_frames * xfecframe_len complex.
    int run_device(const float* d_plframes, int n_frames, int has_trailing_header, const int32_t* d_coarse_corrected,
                   const float* d_coarse_foffset, float* d_out, const PlFrameEstimates& est, hipStream_t stream);
    // the same with frame f in a slot of its own at d_slots + 2 * f * stride_syms floats, stride_syms >= plframe_len + 90: the frame and
    // the 90 symbols that follow it in its stream (what PlSyncBatchHip::gather_device writes), so every frame has its true next header
    int run_strided_device(const float* d_slots, int stride_syms, int n_frames, const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                           float* d_out, const PlFrameEstimates& est, hipStream_t stream);

private:
    int launch(const float* d_plframes, int stride_syms, int n_frames, int has_trailing_header, const int32_t* d_coarse_corrected,
               const float* d_coarse_foffset, float* d_out, const PlFrameEstimates& est, hipStream_t stream);
    PlsInfo pls_{};
    int max_frames_;
    PlPayloadHip* pp_ = nullptr; // owns the Rn table and the payload kernel launch
    float* d_par_ = nullptr;     // what the payload step reads: plheader_phase | phase_inc | pilot_phase
};

} // namespace dvbs2
