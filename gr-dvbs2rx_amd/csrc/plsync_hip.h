// plsync_hip.h -- PLFRAME search on the device: what frame_sync::step (reference lib/pl_frame_sync.cc:66-243) does per
// symbol on a CPU core, as three kernels over a resident symbol buffer.
//   metric   the timing metric of :99-150 for EVERY symbol index: differentials d[n] = conj(x[n]) x[n-1], the 25-tap SOF
//            correlation S over header positions 1..25, the 32-tap PLSC-pair correlation P over positions 27, 29 .. 89,
//            metric[n] = max(|S + P|, |S - P|), peaking on the LAST PLHEADER symbol. The taps are +-j, so S and P are
//            signed sums of swapped components; the signs come from kSofWord and kPlscScrambler at compile time
//            (plsync_tap_bits below) and are checked against plheader_symbols(0) when a handle is created.
//   tracker  the three-state machine of :168-243 in ONE wavefront: while searching / found it scans 64 indices per step
//            with a ballot of metric > 30, once locked it visits one index per frame (metric > 25). At every accepted or
//            inferred peak (:242, lib/plsync_cc_impl.cc:880) the PLSC of the 90 symbols ending there is decoded with the
//            decoder of plsc_decode.hpp (or taken as given in fixed-PLSC mode, lib/plsync_cc_impl.cc:145-159) and sets
//            the frame length (:594).
//   gather   copies the reported locked frames of one PLSC into the back-to-back layout PlFrameHip::run_device reads.
//
// Reserved MODCODs (29..31): pls_info_t::parse gives them the dummy frame's 36 slots (a quarter of that with the short
// bit, plus pilot blocks with the pilot bit; lib/pl_signaling.cc:41-54), so frame_sync::set_frame_len never refuses a
// decoded PLSC (no length exceeds MAX_PLFRAME_LEN). The tracker does the same: it takes pls_parse's length.
//
// One defined difference from the reference: it picks its even or odd PLSC delay line by d_sym_cnt & 1 (:118-121) and
// restarts d_sym_cnt at every peak (:229), so after a peak accepted at an odd count outside lock two consecutive
// differentials land in the same line and its PLSC correlation is not the sliding one for the next 63 symbols. Frame
// lengths are even, so this never happens in lock; outside lock a crossing within 63 symbols of an earlier one (true or false)
// accepted at an odd count can differ. The metric here is the clean sliding correlation everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "device_stage.h"
#include "plframe_hip.h"

namespace dvbs2 {

constexpr float kPlsyncThresholdUnlocked = 30.0f; // threshold_u, lib/pl_frame_sync.h:160
constexpr float kPlsyncThresholdLocked = 25.0f;   // threshold_l, lib/pl_frame_sync.h:162
constexpr int kPlsyncHistory = 89;                // symbols before n that metric[n] and the PLSC decode at n read
constexpr int kPlsyncMinSymbols = 33282 + 90;     // the longest PLFRAME and the header after it

// bit k (1 <= k <= 89) = 1 where the tap of header position k is -j, 0 where it is +j; the tap is the conjugate of the
// expected differential conj(h_k) h_{k-1} of the PLHEADER of PLSC 0. With h_k = (k odd ? -S + jS : S + jS)(1 - 2 b_k)
// (lib/pi2_bpsk.cc:18-43) that differential is (1 - 2 (b_k ^ b_{k-1})) (k odd ? -j : +j). Returned as two words: bits of
// positions 0..63 in lo, 64..89 in hi. Bit 0 of a PLSC complements both bits of every pair's SECOND symbol relative to the
// first, i.e. flips all 32 PLSC taps; no other PLSC bit reaches a within-pair differential.
struct PlsyncTapBits { uint64_t lo, hi; };
constexpr PlsyncTapBits plsync_tap_bits()
{
    PlsyncTapBits t{ 0, 0 };
    for (int k = 1; k < 90; k++) {
        const int flip = plheader_bit(kPlscScrambler, k) ^ plheader_bit(kPlscScrambler, k - 1); // the PLHEADER of PLSC 0
        const int tap_minus = (k & 1) ? flip : !flip; // tap = conj(differential): +j for odd k without a bit flip
        if (tap_minus) { if (k < 64) t.lo |= 1ull << k; else t.hi |= 1ull << (k - 64); }
    }
    return t;
}
// (plsync_taps of pl_signal.h gives the same signs at run time from the 90 expected symbols of PLSC 0)

struct PlSyncFrame { // one detected PLHEADER
    int64_t sof_index; // of the first PLHEADER symbol, counted from reset
    float metric;      // the timing metric on the last PLHEADER symbol
    uint8_t plsc;      // decoded (or the fixed) PLSC
    uint8_t flags;     // bit 0: a real peak (metric above the threshold), not an inferred one; bit 1: locked after this header
    uint8_t reserved[2];
};
static_assert(sizeof(PlSyncFrame) == 16, "record layout");

struct PlSyncState { // lives on the device; read back by finish()
    int64_t abs_base;      // absolute index of symbol 0 of the NEXT buffer
    int64_t last_base;     // ... of the buffer of the last search (what gather's indices are relative to)
    int64_t abs_last_peak; // absolute index of the last peak, -1 after reset: d_sym_cnt at index a is a - abs_last_peak
    int64_t abs_next;      // next index to visit while not locked
    int32_t state, frame_len, unlock_cnt, hist_sel;
    int32_t last_n_syms, last_n_frames, last_consumed;
    int32_t hold;          // abs_base is the resume point of a pending frame: nothing is consumed before that frame is looked at again
};

class PlSyncHip : public PlscListStage {
public:
    // the ranges of the arguments are checked by dvbs2_plsync_create, which alone constructs this
    PlSyncHip(int plsc_or_minus1, int unlock_thresh, int max_symbols, int max_frames, int device);
    int max_symbols() const { return max_symbols_; }
    int max_frames() const { return max_frames_; }
    int reset();
    // DEVICE pointers. metric: n_syms floats, computed with the handle's history, the handle does not advance
    int metric_device(const float* d_syms, int n_syms, float* d_metric, hipStream_t stream);
    // d_frames: max_frames records. Metric, tracker and history update on `stream`; finish() waits and reads the result
    int search_device(const float* d_syms, int n_syms, PlSyncFrame* d_frames, hipStream_t stream);
    int finish(int* n_frames, int* consumed, int* state);
    // d_plframes: room for every selected frame + 90 symbols; d_count: one int32
    int gather_device(const float* d_syms, const PlSyncFrame* d_frames, int n_frames, int wanted_plsc, float* d_plframes,
                      int32_t* d_count, hipStream_t stream);

private:
    int fixed_plsc_, unlock_thresh_, max_symbols_, max_frames_;
    float* d_metric_ = nullptr;     // max_symbols floats
    float2* d_hist_ = nullptr;      // 2 x 89 symbols, the tracker writes the one the state does not select
    PlSyncState* d_state_ = nullptr;
    hipStream_t last_stream_ = nullptr;
};

} // namespace dvbs2
