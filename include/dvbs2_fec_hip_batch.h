/*
 * dvbs2_fec_hip_batch.h -- the part of the C ABI of libdvbs2_fec_hip.so that takes a BATCH of symbol streams from the symbol
 * synchroniser's output to the FEC chain's input: PLFRAME search, gather, coarse frequency estimate and front end for S streams in
 * a fixed number of launches. dvbs2_fec_hip.h includes this file; the conventions (return codes, dvbs2_last_error, DEVICE pointers
 * and a hipStream_t as void* in the "_device" entries, the answer to a null handle) are the ones stated there.
 *
 * The arithmetic is that of the single-stream handles (dvbs2_plsync_*, dvbs2_plcoarse_*, dvbs2_plframe_*), and the device code is
 * shared with them: for every stream, every result here is, bit for bit, what a single-stream handle of its own gives for that
 * stream. The single-stream handles are the specification of this file, and its tests compare against them.
 *
 * The path for S streams, every step asynchronous on one stream, with ONE host wait (dvbs2_plsync_batch_finish, needed only to
 * learn each stream's `consumed`):
 *   dvbs2_symsync_work_device            S rows of symbols (existing)
 *   dvbs2_plsync_batch_search_device     records of every stream                          1 copy of 8 S bytes, 2 launches
 *   dvbs2_plsync_batch_gather_device     slots of plframe_len + 90 symbols, d_offsets     2 launches
 *   dvbs2_plcoarse_batch_estimate_device per-slot coarse_foffset / coarse_corrected        2 launches
 *   dvbs2_plframe_process_strided_device XFECFRAMEs of all slots of all streams            2 launches
 *   dvbs2_chain_*                        one FEC call over all frames (existing)
 */
#ifndef DVBS2_FEC_HIP_BATCH_H
#define DVBS2_FEC_HIP_BATCH_H

#include "dvbs2_fec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched PLFRAME search. One handle holds max_streams independent trackers, each with the state of a dvbs2_plsync_t: machine
 * state, frame length, unlock count, absolute offset, resume point and the 89 symbols before its consumed point. plsc_or_minus1,
 * unlock_thresh, max_symbols (per stream) and max_frames (per stream) are as for dvbs2_plsync_create; max_streams is 1..1024.
 * set_plsc_mode and set_expected_pls act on the whole handle. dvbs2_plsync_batch_reset gives every stream as created,
 * dvbs2_plsync_batch_reset_stream one stream; both wait for the device.
 *
 * dvbs2_plsync_batch_search_device: stream s reads n_syms[s] symbols from d_syms + 2 * (s * stride_syms + first[s]) floats. first and
 * n_syms are HOST arrays of n_streams ints; the call takes its copy of them before it returns, as dvbs2_symsync_work_device does with
 * n_in. first[s] lets every stream be presented again from its own `consumed` without a copy. n_syms[s] == 0 is legal and leaves
 * stream s untouched: it reports no frame, consumes nothing, and its state is the one it had. With more than one stream a row must
 * not run into the next (first[s] + n_syms[s] <= stride_syms). d_syms must be 8-byte aligned. d_frames is [n_streams][max_frames]
 * records of dvbs2_plsync_frame_t, stream s's at d_frames + s * max_frames. Two launches for any number of streams: the timing metric
 * over a (tile, stream) grid, then one wavefront per stream. dvbs2_plsync_batch_finish waits for the last search and fills arrays of
 * that search's n_streams ints (each nullable): one wait, one copy.
 *
 * dvbs2_plsync_batch_gather_device refers to the buffers of the LAST search, including that search's first[] (d_syms and stride_syms
 * are passed again, as dvbs2_plsync_gather_device takes d_syms again); n_streams is at most that search's. Every reported frame that
 * is locked and carries wanted_plsc is copied into a SLOT of plframe_len + 90 symbols: the frame and the 90 symbols that follow it in
 * its own stream (the buffer-end rule guarantees they lie inside the buffer). Slots are stream-major and in stream order within a
 * stream. d_offsets[0 .. n_streams] (int32) receives the prefix sums of the selected counts: stream s owns slots d_offsets[s] ..
 * d_offsets[s + 1]. These are the true counts even above max_slots; slots with index >= max_slots are not written. d_slot_record is
 * nullable; when given, slot i receives its (stream, record index) as two int32. d_slots should be 16-byte aligned. Every slot
 * carries its own next header, so slots of any streams can share one dvbs2_plframe_*_strided_device launch, and a pilotless front
 * end sees the true next header also when other frames lie between two gathered ones.
 *
 * dvbs2_plsync_batch_check (host only) holds the argument ranges of create; dvbs2_plsync_batch_check_search (host only) those of a
 * search against a handle's max_streams and max_symbols: the two entries call them first. */
typedef struct dvbs2_plsync_batch dvbs2_plsync_batch_t;
int dvbs2_plsync_batch_check(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames);
int dvbs2_plsync_batch_check_search(int max_streams, int max_symbols, int64_t stride_syms, const int* first, const int* n_syms, int n_streams);
int dvbs2_plsync_batch_create(dvbs2_plsync_batch_t** h, int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames,
                              int device);
void dvbs2_plsync_batch_destroy(dvbs2_plsync_batch_t* h);
int dvbs2_plsync_batch_reset(dvbs2_plsync_batch_t* h);
int dvbs2_plsync_batch_reset_stream(dvbs2_plsync_batch_t* h, int stream_index);
int dvbs2_plsync_batch_set_plsc_mode(dvbs2_plsync_batch_t* h, int coherent, int soft);
int dvbs2_plsync_batch_set_expected_pls(dvbs2_plsync_batch_t* h, const uint8_t* plsc_list, int n);
int dvbs2_plsync_batch_search_device(dvbs2_plsync_batch_t* h, const float* d_syms, int64_t stride_syms, const int* first, const int* n_syms,
                                     int n_streams, dvbs2_plsync_frame_t* d_frames, void* stream);
int dvbs2_plsync_batch_finish(dvbs2_plsync_batch_t* h, int* n_frames, int* consumed, int* state);
int dvbs2_plsync_batch_gather_device(dvbs2_plsync_batch_t* h, const float* d_syms, int64_t stride_syms, const dvbs2_plsync_frame_t* d_frames,
                                     int n_streams, int wanted_plsc, float* d_slots, int max_slots, int32_t* d_offsets, int32_t* d_slot_record,
                                     void* stream);

/* ---- strided PLFRAME front end: dvbs2_plframe_estimate_device / dvbs2_plframe_process_device with frame f at symbol f * stride_syms
 * of d_slots and its next header inside its slot, stride_syms >= plframe_len + 90 (dvbs2_plframe_stride_check, host only, holds the
 * rule). Every frame has a next header, so there is no has_trailing_header. The back-to-back entries are this with stride
 * plframe_len and keep their bits. */
int dvbs2_plframe_stride_check(int plsc, int64_t stride_syms);
int dvbs2_plframe_estimate_strided_device(dvbs2_plframe_t* h, const float* d_slots, int64_t stride_syms, int n_frames,
                                          const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                                          const dvbs2_plframe_estimates_t* d_est, void* stream);
int dvbs2_plframe_process_strided_device(dvbs2_plframe_t* h, const float* d_slots, int64_t stride_syms, int n_frames,
                                         const int32_t* d_coarse_corrected, const float* d_coarse_foffset, float* d_xfecframes,
                                         const dvbs2_plframe_estimates_t* d_est, void* stream);

/* ---- batched coarse frequency estimate: dvbs2_plcoarse_estimate_device over the slots of a gather, with one window state per
 * stream. period and plsc_or_minus1 as for dvbs2_plcoarse_create; max_streams 1..1024; max_slots 1..1048576. The autocorrelation
 * runs over max_slots wavefronts, of which those at or beyond d_offsets[n_streams] leave at once; then one wavefront per stream walks
 * slots d_offsets[s] .. d_offsets[s + 1] (those below max_slots) in order over its own state. d_offsets is read on the DEVICE: no host
 * round trip lies between gather and estimate. d_plsc: one byte per slot, or NULL for the handle's fixed PLSC. The outputs are per
 * slot, each nullable: exactly the arrays dvbs2_plframe_*_strided_device reads. A stream without a slot in a call keeps its state.
 * d_slots and the outputs must have room for min(d_offsets[n_streams], max_slots) slots: give the gather the handle's max_slots, or less.
 * dvbs2_plcoarse_batch_reset / _reset_stream wait for the device. */
typedef struct dvbs2_plcoarse_batch dvbs2_plcoarse_batch_t;
int dvbs2_plcoarse_batch_create(dvbs2_plcoarse_batch_t** h, int period, int plsc_or_minus1, int max_streams, int max_slots, int device);
void dvbs2_plcoarse_batch_destroy(dvbs2_plcoarse_batch_t* h);
int dvbs2_plcoarse_batch_reset(dvbs2_plcoarse_batch_t* h);
int dvbs2_plcoarse_batch_reset_stream(dvbs2_plcoarse_batch_t* h, int stream_index);
int dvbs2_plcoarse_batch_estimate_device(dvbs2_plcoarse_batch_t* h, const float* d_slots, int64_t stride_syms, const uint8_t* d_plsc,
                                         const int32_t* d_offsets, int n_streams, float* d_coarse_foffset, int32_t* d_coarse_corrected,
                                         int32_t* d_new_est, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVBS2_FEC_HIP_BATCH_H */
