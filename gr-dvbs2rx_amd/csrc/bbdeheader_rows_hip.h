// bbdeheader_rows_hip.h -- the BBFRAME de-header for a batch of streams from state held in DEVICE memory (include/dvbs2_fec_hip.h,
// "de-header rows"; notes/bbdeheader_rows.md).
//   A stream's state is one 256-byte record in the caller's device memory: the block's synchronised flag, the carried partial packet and
//   the six counters. Stream s owns the BBFRAMEs d_offsets[s] .. d_offsets[s + 1] of one buffer, as dvbs2_plsync_batch_gather_device
//   counts them and dvbs2_chain_* writes them; the offsets are read on the device. What a stream emits and what its record holds
//   afterwards are the single handle's (bbdeheader_hip.h) fed the same frames: the device code is the same (bbdeheader_device.hpp).
//   All-zero bytes are the block as constructed.
// There is no handle, no allocation and no host synchronisation here; the five launches are asynchronous on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "bbdeheader_hip.h"

namespace dvbs2 {

struct BbdhRow { // dvbs2_bbdeheader_state_t
    int synched, partial;
    unsigned long long packets, errors, bbframes, dropped, gaps, overruns;
    int last_packets, reserved; // packets of the last call that touched the record
    unsigned char partial_pkt[kTsLen];
    unsigned char pad[4];
};
static_assert(sizeof(BbdhRow) == 256, "the record is 256 bytes");

constexpr int kBbdhRowsMaxStreams = 1024;    // the gather that writes d_offsets
constexpr int kBbdhRowsMaxFrames = 1 << 20;
constexpr int kBbdhMaxPacketsPerFrame = 64;  // the packet kernel's workgroup

// "" or what is wrong, naming the argument: BbDeheaderHip's rules for kbch_bits, n_streams 1..1024, max_frames 1..2^20
std::string bbdeheader_rows_check(int kbch_bits, int n_streams, int max_frames);

struct BbdhRowsGeometry {
    int kbch_bytes, max_dfl, max_out_bytes_per_frame;
    int64_t hdr_at, map_at, plan_at, tail_at; // byte offsets into the workspace, 16-byte aligned
    int64_t work_bytes, out_bytes;
};
BbdhRowsGeometry bbdeheader_rows_geometry(int kbch_bits, int n_streams, int max_frames); // of arguments that pass the check

// Five launches on `stream` of the current device; the hipError_t of the last. Arguments are the C entry's, already checked.
hipError_t bbdeheader_rows_launch(const uint8_t* d_bbframes, int kbch_bits, const int32_t* d_offsets, int n_streams, int max_frames, BbdhRow* d_state,
                                  void* d_work, uint8_t* d_ts_out, int64_t out_bytes, int32_t* d_pkt_offsets, hipStream_t stream);

} // namespace dvbs2
