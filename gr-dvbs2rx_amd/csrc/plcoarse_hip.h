// plcoarse_hip.h -- coarse frequency offset estimate on the device: freq_sync::estimate_coarse (reference
// lib/pl_freq_sync.cc:93-199) with the mode rule of its caller (lib/plsync_cc_impl.cc:567-606), as two kernels.
//   autocorr  one wavefront per PLHEADER, no LDS, no barrier: the modulation is removed with swaps and signs
//             (z[k] = x[k] conj(h[k]) sqrt(2): h is pi/2 BPSK, the common scale does not reach an angle), the 90 values stay
//             in registers, and lane m forms lag m and its complement 90 - m in ONE pass of 90 steps: at step u it takes
//             z[(u + m) mod 90] against z[u], which is a term of lag m while u + m < 90 and a term of lag 90 - m after the
//             wrap. The SOF form (N = 26) is the same pass over 26 steps. BOTH forms are written for every frame, so this
//             kernel does not depend on the estimator's state.
//   window    one wavefront walks the frames in order, lanes over lags: it adds the form the state selects, and on the last
//             frame of a window takes the 89 (25) angles, their differences (__shfl_up), the wrap, the weights and a
//             butterfly sum, clips, sets the coarse-corrected flag and clears the accumulator.
// A frame uses the full PLHEADER when the state was coarse-corrected before it or the handle was created with a known PLSC
// (the reference's "PLSC decoder disabled"), the SOF otherwise; the state changes only on a window's last frame.
//
// Accuracy: float sums in a fixed order where the reference uses VOLK's dot product, atan2f where it uses gr::fast_atan2f
// (a table). Neither is available to pin against, so the estimate is tested against a float64 model under a derived bound
// (tests/plcoarse_model.py) and is UNPINNED against the genuine reference, like the other float paths of this library.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "device_stage.h"
#include "plsync_hip.h"
#include "plsync_batch_hip.h"

namespace dvbs2 {

constexpr double kFineFoffsetCorrRange = 3.3875e-4; // lib/pl_freq_sync.h:18
constexpr int kPlcoarseRecord = 90 + 26;            // float2 per frame between the kernels: R_full[0..89] | R_sof[0..25]

struct PlCoarseState { // lives on the device
    float2 acc[90];    // pilot_corr[1..L] at [1..L]
    int32_t i_frame, corrected;
    float foffset;
    int32_t reserved;
};

// per-frame outputs, DEVICE pointers, each nullable
struct PlCoarseOut {
    float* foffset = nullptr;     // the latest estimate (0 before the first)
    int32_t* corrected = nullptr; // the state after this frame
    int32_t* new_est = nullptr;   // 1 on the last frame of a window
};

class PlCoarseHip : public DeviceStage {
public:
    // the ranges of the arguments are checked by dvbs2_plcoarse_create, which alone constructs this
    PlCoarseHip(int period, int plsc_or_minus1, int max_frames, int device);
    int max_frames() const { return max_frames_; }
    int fixed_plsc() const { return fixed_plsc_; }
    int reset();
    // DEVICE pointers. Frame f starts at d_plframes + 2 * f * stride_syms floats; d_plsc: one byte per frame, or null for
    // the handle's fixed PLSC (the caller has checked that one of the two is there and that stride_syms >= 90)
    int frames_device(const float* d_plframes, int64_t stride_syms, const uint8_t* d_plsc, int n_frames, const PlCoarseOut& out,
                      hipStream_t stream);
    // d_syms[0] has absolute index `base`; record f names the header at sof_index - base and its PLSC. A record whose 90
    // symbols are not all inside [0, n_syms) is passed over: it is no frame of the window, its outputs repeat the state
    int records_device(const float* d_syms, int n_syms, const PlSyncFrame* d_records, int n_frames, int64_t base, const PlCoarseOut& out,
                       hipStream_t stream);

private:
    int launch(const float2* x, int64_t stride, const uint8_t* plsc, const PlSyncFrame* rec, int n_syms, int64_t base, int n_frames,
               const PlCoarseOut& out, hipStream_t stream);
    int period_, fixed_plsc_, max_frames_;
    uint64_t* d_cw_ = nullptr;   // 128 scrambled PLSC codewords
    float* d_w_ = nullptr;       // 89 + 25 window weights
    float2* d_r_ = nullptr;      // max_frames * kPlcoarseRecord
    PlCoarseState* d_state_ = nullptr;
};

// host only: empty when the arguments of a batch create are in range, else what is wrong (always an argument error)
std::string plcoarse_batch_check(int period, int plsc_or_minus1, int max_streams, int max_slots);

// The same estimate for the slots PlSyncBatchHip::gather_device writes (plsync_batch_hip.h): one PlCoarseState per stream. The
// autocorrelation runs over every slot; stream s's wavefront walks slots d_offsets[s] .. d_offsets[s + 1] in order, so its outputs
// are the bits a PlCoarseHip of its own gives for those slots. d_offsets is read on the device: no host round trip lies between
// gather and estimate. Slots at or beyond max_slots are not looked at (gather has not written them).
class PlCoarseBatchHip : public DeviceStage {
public:
    // the ranges of the arguments are checked by dvbs2_plcoarse_batch_create (plcoarse_batch_check), which alone constructs this
    PlCoarseBatchHip(int period, int plsc_or_minus1, int max_streams, int max_slots, int device);
    int max_streams() const { return max_streams_; }
    int max_slots() const { return max_slots_; }
    int fixed_plsc() const { return fixed_plsc_; }
    int reset();
    int reset_stream(int s);
    // DEVICE pointers. Slot i starts at d_slots + 2 * i * stride_syms floats; d_plsc: one byte per slot, or null for the handle's
    // fixed PLSC; d_offsets: n_streams + 1 int32 prefix sums; the outputs are per slot
    int slots_device(const float* d_slots, int64_t stride_syms, const uint8_t* d_plsc, const int32_t* d_offsets, int n_streams, const PlCoarseOut& out,
                     hipStream_t stream);

private:
    int clear(int first_stream, int count);
    int period_, fixed_plsc_, max_streams_, max_slots_;
    uint64_t* d_cw_ = nullptr;   // 128 scrambled PLSC codewords
    float* d_w_ = nullptr;       // 89 + 25 window weights
    float2* d_r_ = nullptr;      // max_slots * kPlcoarseRecord
    PlCoarseState* d_state_ = nullptr; // [max_streams]
};

} // namespace dvbs2
