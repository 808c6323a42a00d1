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
#include "plsc_decode.hpp" // kSofWord, kPlscScrambler and the one-wavefront PLSC decoder

namespace dvbs2 {

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

// device (or host-staged) outputs of the estimate kernel, each nullable
struct PlFrameEstimates {
    uint8_t* plsc_decoded = nullptr;
    float* sof_phase = nullptr;
    float* plheader_phase = nullptr;
    float* pilot_phase = nullptr;
    float* fine_foffset = nullptr;
    int32_t* fine_valid = nullptr;
};

class PlFrameHip : public DeviceStage {
public:
    // plsc is checked by dvbs2_plframe_create, which alone constructs this: within 0..127 and no reserved MODCOD
    PlFrameHip(int gold_code, int plsc, int max_frames, int device);
    ~PlFrameHip();
    const PlsInfo& pls() const { return pls_; }
    int max_frames() const { return max_frames_; }
    void set_plsc_mode(int coherent, int soft) { coherent_ = coherent ? 1 : 0; soft_ = soft ? 1 : 0; }
    // the enabled-codeword list of the reference's second plsc_decoder constructor, in the caller's order (n = 0: all 128)
    int set_expected_pls(const uint8_t* list, int n);
    // DEVICE pointers. d_plframes: n_frames * plframe_len complex (+ 90 when has_trailing_header); d_coarse_corrected:
    // n_frames int32; d_coarse_foffset: n_frames float, needed only by pilotless handles. d_out (nullable = estimates
    // only): n_frames * xfecframe_len complex.
    int run_device(const float* d_plframes, int n_frames, int has_trailing_header, const int32_t* d_coarse_corrected,
                   const float* d_coarse_foffset, float* d_out, const PlFrameEstimates& est, hipStream_t stream);

private:
    PlsInfo pls_{};
    int max_frames_, coherent_ = 1, soft_ = 1;
    PlPayloadHip* pp_ = nullptr; // owns the Rn table and the payload kernel launch
    uint8_t* d_rank_ = nullptr;  // 128 bytes: position of each codeword in the enabled list, 255 = disabled
    float* d_par_ = nullptr;     // what the payload step reads: plheader_phase | phase_inc | pilot_phase
};

} // namespace dvbs2
