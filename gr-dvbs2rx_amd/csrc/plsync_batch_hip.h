// plsync_batch_hip.h -- the PLFRAME search of plsync_hip.h for a batch of independent symbol streams in one handle: S streams
// cost the launches of one. The arithmetic is plsync_device.hpp's, which the single-stream kernels run too, so stream s of a batch
// gives the bits a PlSyncHip of its own gives for that stream.
//   metric   a (tile, stream) grid; a block beyond its stream's length leaves at once.
//   tracker  one wavefront per stream in ONE launch, each over its own PlSyncState and 2 x 89 symbol history.
//   gather   one workgroup counts the selected records of every stream and writes the prefix sums; then one workgroup per record
//            copies a selected frame AND the 90 symbols behind it in its own stream into a slot of plframe_len + 90 symbols. Every
//            slot carries its own next header, so slots of any streams can share one strided front-end launch (plframe_hip.h).
// A stream with n_syms[s] == 0 is not touched: state, history and absolute offset stay, it reports no frame and consumes nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "plsync_hip.h"

namespace dvbs2 {

constexpr int kPlsyncBatchMaxStreams = 1024;

// host only: empty when the arguments of a create are in range, else what is wrong (always an argument error)
std::string plsync_batch_check(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames);

struct PlSyncBatchResult { int32_t n_frames, consumed, state, n_syms; }; // of the last search, per stream; lives on the device
struct PlSyncBatchCall { int32_t first, n_syms; };                       // the last search's view of a stream, uploaded per call

class PlSyncBatchHip : public PlscListStage {
public:
    // the ranges of the arguments are checked by dvbs2_plsync_batch_create (plsync_batch_check), which alone constructs this
    PlSyncBatchHip(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames, int device);
    int max_streams() const { return max_streams_; }
    int max_symbols() const { return max_symbols_; }
    int max_frames() const { return max_frames_; }
    int reset();
    int reset_stream(int s);
    // d_syms: DEVICE; first, n_syms: HOST arrays of n_streams (the caller has checked their ranges). Stream s reads n_syms[s] symbols
    // from d_syms + 2 * (s * stride_syms + first[s]). d_frames: [n_streams][max_frames] records
    int search_device(const float* d_syms, int64_t stride_syms, const int* first, const int* n_syms, int n_streams, PlSyncFrame* d_frames,
                      hipStream_t stream);
    // arrays of the last search's n_streams, each nullable; returns that n_streams, or -1
    int finish(int* n_frames, int* consumed, int* state);
    // the LAST search's buffers. d_slots: max_slots * (plframe_len + 90) symbols; d_offsets: n_streams + 1 int32; d_slot_record:
    // nullable, 2 int32 per slot
    int gather_device(const float* d_syms, int64_t stride_syms, const PlSyncFrame* d_frames, int n_streams, int wanted_plsc, float* d_slots,
                      int max_slots, int32_t* d_offsets, int32_t* d_slot_record, hipStream_t stream);

private:
    int write_fresh(int first_stream, int count);
    int fixed_plsc_, unlock_thresh_, max_streams_, max_symbols_, max_frames_;
    float* d_metric_ = nullptr;          // [max_streams][max_symbols]
    float2* d_hist_ = nullptr;           // [max_streams][2][89]
    PlSyncState* d_state_ = nullptr;     // [max_streams]
    PlSyncBatchCall* d_call_ = nullptr;  // [max_streams]
    PlSyncBatchResult* d_res_ = nullptr; // [max_streams]
    std::vector<PlSyncBatchCall> call_;
    std::vector<PlSyncBatchResult> res_;
    int last_streams_ = 0, last_max_n_ = 0;
    hipStream_t last_stream_ = nullptr;
};

} // namespace dvbs2
