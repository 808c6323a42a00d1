// bbdeheader_rows_hip.hip -- see bbdeheader_rows_hip.h. Five launches per call, for any number of streams:
//   1  bbdh_rows_header_kernel  one thread per frame over max_frames: the header word of every frame below the call's frame count, and
//                               "no stream" in the frame-to-stream map
//   2  bbdh_rows_scan_kernel    one workgroup per stream: the state machine of bbdeheader_device.hpp over the stream's frames and record;
//                               also the stream's tail plan (with its packet count) and the stream index of each of its frames
//   3  bbdh_rows_prefix_kernel  one workgroup: the exclusive prefix of the packet counts into d_pkt_offsets
//   4  bbdh_rows_packet_kernel  one workgroup per frame over max_frames: gather, CRC-8 and sync byte, behind its stream's d_pkt_offsets
//   5  bbdh_rows_save_kernel    one workgroup per stream: the carried partial packet, after every reader of the old one
// The frame ranges come from d_offsets on the device. Whatever it holds, nothing leaves the buffers: every offset is clamped to
// [0, frames of the call], a pair that does not increase is an empty stream, and a plan is used only if it lies inside its frame, its
// stream's range and the output (with offsets that do not decrease every plan does, by construction of the scan; ranges that overlap
// make two workgroups write the same plans, and the result for those streams is then undefined, inside the buffers).
#include "bbdeheader_rows_hip.h"
#include <algorithm>

namespace dvbs2 {

__device__ __forceinline__ void bbdh_set_last(BbdhRow* st, int out_pkts) { st->last_packets = out_pkts; }

} // namespace dvbs2

#include "bbdeheader_device.hpp"

namespace dvbs2 {

std::string bbdeheader_rows_check(int kbch_bits, int n_streams, int max_frames)
{
    if (kbch_bits < 88 || kbch_bits % 8 != 0 || kbch_bits - 80 > 0xffff) return "kbch_bits must be a multiple of 8 in 88..65615";
    if (((kbch_bits - 80) / 8 + kTsLen - 1) / kTsLen > kBbdhMaxPacketsPerFrame) return "kbch_bits gives more than 64 packets per BBFRAME";
    if (n_streams < 1 || n_streams > kBbdhRowsMaxStreams) return "n_streams out of range (1..1024)";
    if (max_frames < 1 || max_frames > kBbdhRowsMaxFrames) return "max_frames out of range (1..2^20)";
    return "";
}

BbdhRowsGeometry bbdeheader_rows_geometry(int kbch_bits, int n_streams, int max_frames)
{
    const auto align16 = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
    BbdhRowsGeometry g;
    g.kbch_bytes = kbch_bits / 8;
    g.max_dfl = kbch_bits - 80;
    g.max_out_bytes_per_frame = (g.max_dfl / 8 + kTsLen - 1) / kTsLen * kTsLen;
    g.hdr_at = 0;
    g.map_at = g.hdr_at + align16((int64_t)max_frames * sizeof(int));
    g.plan_at = g.map_at + align16((int64_t)max_frames * sizeof(int));
    g.tail_at = g.plan_at + align16((int64_t)max_frames * sizeof(BbdhPlan));
    g.work_bytes = g.tail_at + align16((int64_t)n_streams * sizeof(BbdhPlan));
    g.out_bytes = (int64_t)max_frames * g.max_out_bytes_per_frame;
    return g;
}

namespace {

// the frames of the call: d_offsets[n_streams], at most max_frames
__device__ __forceinline__ int rows_total(const int32_t* __restrict__ offsets, int n_streams, int max_frames)
{
    return min(max(offsets[n_streams], 0), max_frames);
}
// the frames [lo, hi) of stream s; hi <= lo: none
__device__ __forceinline__ void rows_range(const int32_t* __restrict__ offsets, int s, int n_streams, int max_frames, int* lo, int* hi)
{
    const int total = rows_total(offsets, n_streams, max_frames);
    *lo = min(max(offsets[s], 0), total);
    *hi = min(max(offsets[s + 1], 0), total);
}

__global__ __launch_bounds__(256) void bbdh_rows_header_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ offsets, int n_streams,
                                                                int max_frames, int kbch_bytes, int max_dfl, int* __restrict__ hdr, int* __restrict__ map)
{
    __shared__ uint8_t tab[256];
    crc8_build(tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= max_frames) return;
    map[f] = -1;
    if (f >= rows_total(offsets, n_streams, max_frames)) return;
    hdr[f] = bbdh_header_word(in + (size_t)f * kbch_bytes, max_dfl, tab);
}

__global__ __launch_bounds__(kScanThreads) void bbdh_rows_scan_kernel(const int32_t* __restrict__ offsets, int n_streams, int max_frames,
                                                                       const int* __restrict__ hdr, BbdhRow* __restrict__ state,
                                                                       BbdhPlan* __restrict__ plan, BbdhPlan* __restrict__ tails, int* __restrict__ map)
{
    const int s = blockIdx.x;
    int lo, hi;
    rows_range(offsets, s, n_streams, max_frames, &lo, &hi);
    if (hi <= lo) { // no frame: the record is not touched
        if (threadIdx.x == 0) { BbdhPlan t; t.src_off = 0; t.head = 0; t.head_frame = -1; t.head_off = 0; t.n_pkts = 0; t.out_base = 0; tails[s] = t; }
        return;
    }
    for (int f = lo + threadIdx.x; f < hi; f += kScanThreads) map[f] = s;
    bbdh_scan_stream(hdr + lo, hi - lo, state + s, plan + lo, tails + s);
}

__global__ __launch_bounds__(kScanThreads) void bbdh_rows_prefix_kernel(const BbdhPlan* __restrict__ tails, int n_streams, int32_t* __restrict__ pkt_offsets)
{
    __shared__ int sh[kScanThreads];
    const int tid = threadIdx.x;
    const int per = (n_streams + kScanThreads - 1) / kScanThreads;
    const int c0 = min(tid * per, n_streams), c1 = min(c0 + per, n_streams);
    int sum = 0;
    for (int s = c0; s < c1; s++) sum += tails[s].out_base;
    int total;
    int at = block_excl_scan(sum, sh, tid, &total);
    for (int s = c0; s < c1; s++) { pkt_offsets[s] = at; at += tails[s].out_base; }
    if (tid == 0) pkt_offsets[n_streams] = total;
}

__global__ __launch_bounds__(kBbdhMaxPacketsPerFrame) void bbdh_rows_packet_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ offsets,
                                                                                    int n_streams, int max_frames, int kbch_bytes, BbdhRow* __restrict__ state,
                                                                                    const BbdhPlan* __restrict__ plan, const int* __restrict__ map,
                                                                                    const int32_t* __restrict__ pkt_offsets, uint8_t* __restrict__ out, int64_t out_pkts_room)
{
    const int g = blockIdx.x;
    const int s = map[g];
    if (s < 0 || s >= n_streams) return; // no stream owns the frame
    int lo, hi;
    rows_range(offsets, s, n_streams, max_frames, &lo, &hi);
    if (g < lo || g >= hi) return;
    const BbdhPlan pl = plan[g];
    const int f = g - lo, first = pkt_offsets[s];
    // inside the frame, the stream's frames and the output, or nothing (uniform over the workgroup)
    if (pl.n_pkts <= 0 || pl.n_pkts > kBbdhMaxPacketsPerFrame || pl.head < 0 || pl.head >= kTsLen || pl.src_off < 0 ||
        (int64_t)pl.src_off + (int64_t)pl.n_pkts * kTsLen - pl.head > kbch_bytes) return;
    if (pl.head > 0 && pl.head_frame >= 0 && (pl.head_frame >= f || pl.head_off < 0 || pl.head_off + pl.head > kbch_bytes)) return;
    if (first < 0 || pl.out_base < 0 || (int64_t)first + pl.out_base + pl.n_pkts > out_pkts_room) return;
    bbdh_frame_packets(in + (size_t)lo * kbch_bytes, f, kbch_bytes, state + s, pl, out + (size_t)first * kTsLen);
}

__global__ __launch_bounds__(192) void bbdh_rows_save_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ offsets, int n_streams, int max_frames,
                                                              int kbch_bytes, BbdhRow* __restrict__ state, const BbdhPlan* __restrict__ tails)
{
    const int s = blockIdx.x;
    const BbdhPlan t = tails[s];
    int lo, hi;
    rows_range(offsets, s, n_streams, max_frames, &lo, &hi);
    if (t.head_frame < 0 || t.head_frame >= hi - lo || t.head < 0 || t.head >= kTsLen || t.src_off < 0 || t.src_off + t.head > kbch_bytes) return;
    bbdh_save_partial(in + (size_t)lo * kbch_bytes, kbch_bytes, state + s, t);
}

} // namespace

hipError_t bbdeheader_rows_launch(const uint8_t* d_bbframes, int kbch_bits, const int32_t* d_offsets, int n_streams, int max_frames, BbdhRow* d_state,
                                  void* d_work, uint8_t* d_ts_out, int64_t out_bytes, int32_t* d_pkt_offsets, hipStream_t stream)
{
    const BbdhRowsGeometry g = bbdeheader_rows_geometry(kbch_bits, n_streams, max_frames);
    char* w = static_cast<char*>(d_work);
    int* hdr = reinterpret_cast<int*>(w + g.hdr_at);
    int* map = reinterpret_cast<int*>(w + g.map_at);
    BbdhPlan* plan = reinterpret_cast<BbdhPlan*>(w + g.plan_at);
    BbdhPlan* tails = reinterpret_cast<BbdhPlan*>(w + g.tail_at);
    hipLaunchKernelGGL(bbdh_rows_header_kernel, dim3((max_frames + 255) / 256), dim3(256), 0, stream, d_bbframes, d_offsets, n_streams, max_frames,
                       g.kbch_bytes, g.max_dfl, hdr, map);
    hipLaunchKernelGGL(bbdh_rows_scan_kernel, dim3(n_streams), dim3(kScanThreads), 0, stream, d_offsets, n_streams, max_frames, hdr, d_state, plan, tails, map);
    hipLaunchKernelGGL(bbdh_rows_prefix_kernel, dim3(1), dim3(kScanThreads), 0, stream, tails, n_streams, d_pkt_offsets);
    hipLaunchKernelGGL(bbdh_rows_packet_kernel, dim3(max_frames), dim3(kBbdhMaxPacketsPerFrame), 0, stream, d_bbframes, d_offsets, n_streams, max_frames,
                       g.kbch_bytes, d_state, plan, map, d_pkt_offsets, d_ts_out, out_bytes / kTsLen);
    hipLaunchKernelGGL(bbdh_rows_save_kernel, dim3(n_streams), dim3(192), 0, stream, d_bbframes, d_offsets, n_streams, max_frames, g.kbch_bytes, d_state, tails);
    return hipGetLastError();
}

} // namespace dvbs2
