// bbdeheader_hip.hip -- see bbdeheader_hip.h. The kernels' bodies are bbdeheader_device.hpp's, shared with the rows. Per call:
//   1  bbdh_header_kernel   one thread per BBFRAME: CRC-8 over the ten header bytes, field checks (parse_bbheader)
//   2  bbdh_scan_kernel     the block's state machine (synched / partial count, gap and resync rules, general_work :160-247) reduced to
//                           what it decides -- where packets start, how many, where the head of a packet that straddles two BBFRAMEs
//                           lies. One workgroup: the healthy prefix of the call as two prefix sums over 256 threads (verified frame by
//                           frame), the rest (from the first gap / bad header / resync on) in order on one thread.
//   3  bbdh_packet_kernel   one workgroup per BBFRAME, one thread per TS packet: gather (at most two pieces), CRC-8, restore
//                           the sync byte, set the transport error indicator on a failed check.
//   4  bbdh_save_partial_kernel  the partial packet for the next call, after every reader of the old one has finished
// The byte work is tiny next to the decoders in front of it (kbch / 8 bytes per frame in, about as many out): no tuning beyond
// keeping everything on the device and asynchronous.
#include "bbdeheader_hip.h"
#include "bbdeheader_device.hpp"

namespace dvbs2 {

__device__ __forceinline__ void bbdh_set_last(BbdhState* st, int out_pkts)
{
    st->n_out_packets = out_pkts; st->produced = (long long)out_pkts * kTsLen;
}

__global__ void bbdh_header_kernel(const uint8_t* __restrict__ in, int n_frames, int kbch_bytes, int max_dfl, int* __restrict__ hdr)
{
    __shared__ uint8_t tab[256];
    crc8_build(tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    hdr[f] = bbdh_header_word(in + (size_t)f * kbch_bytes, max_dfl, tab);
}

// one workgroup; the tail plan travels in the plan slot one past the last frame
__global__ __launch_bounds__(kScanThreads) void bbdh_scan_kernel(const int* __restrict__ hdr, int n_frames, int kbch_bytes, BbdhState* __restrict__ st, BbdhPlan* __restrict__ plan)
{
    bbdh_scan_stream(hdr, n_frames, st, plan, plan + n_frames);
}

__global__ void bbdh_packet_kernel(const uint8_t* __restrict__ in, int n_frames, int kbch_bytes, BbdhState* __restrict__ st,
                                   const BbdhPlan* __restrict__ plan, uint8_t* __restrict__ out)
{
    bbdh_frame_packets(in, (int)blockIdx.x, kbch_bytes, st, plan[blockIdx.x], out);
}

__global__ void bbdh_save_partial_kernel(const uint8_t* __restrict__ in, int n_frames, int kbch_bytes, BbdhState* __restrict__ st, const BbdhPlan* __restrict__ plan)
{
    bbdh_save_partial(in, kbch_bytes, st, plan[n_frames]);
}

BbDeheaderHip::BbDeheaderHip(int kbch_bits, int max_frames, int device)
    : DeviceStage(device), kbch_bytes_(kbch_bits / 8), max_dfl_(kbch_bits - 80), max_frames_(max_frames)
{
    if (kbch_bits < 88 || kbch_bits % 8 != 0 || kbch_bits - 80 > 0xffff) { err_.argument("unsupported BCH message length"); return; }
    if (max_frames_ < 1 || max_frames_ > 65535) { err_.argument("max_frames must be in 1..65535"); return; }
    if (max_out_bytes_per_frame() / kTsLen > 64) { err_.argument("more than 64 packets per BBFRAME"); return; }
    DeviceGuard guard(device_);
    if (!guard.ok) { err_.argument("hipSetDevice failed"); return; } // (device failure, kArgument: notes/stage_error_codes.md)
    hipError_t e = alloc(&d_state_, 1);
    if (e == hipSuccess) e = memset_done(d_state_, 0, sizeof(BbdhState));
    if (e == hipSuccess) e = alloc(&d_plan_, (size_t)max_frames_ + 1);
    if (e == hipSuccess) e = alloc(&d_hdr_, max_frames_);
    hip_ok(e, "bbdeheader buffers", err_, kArgument); // (device failure, kArgument: notes/stage_error_codes.md)
}

int BbDeheaderHip::process_device(const uint8_t* d_bbframes, int n_frames, uint8_t* d_out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    hipLaunchKernelGGL(bbdh_header_kernel, dim3((n_frames + 255) / 256 + (n_frames == 0)), dim3(256), 0, stream, d_bbframes, n_frames, kbch_bytes_, max_dfl_, d_hdr_);
    hipLaunchKernelGGL(bbdh_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_hdr_, n_frames, kbch_bytes_, d_state_, d_plan_);
    if (n_frames > 0) {
        hipLaunchKernelGGL(bbdh_packet_kernel, dim3(n_frames), dim3(64), 0, stream, d_bbframes, n_frames, kbch_bytes_, d_state_, d_plan_, d_out);
        hipLaunchKernelGGL(bbdh_save_partial_kernel, dim3(1), dim3(192), 0, stream, d_bbframes, n_frames, kbch_bytes_, d_state_, d_plan_);
    }
    return launched("bbdeheader launch");
}

int BbDeheaderHip::state(BbdhState* out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    hipError_t e = hipMemcpyAsync(out, d_state_, sizeof(BbdhState), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return hip_ok(e, "bbdeheader state", call_err_) ? 0 : -1;
}

int BbDeheaderHip::reset(hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    hipError_t e = hipMemsetAsync(d_state_, 0, sizeof(BbdhState), stream);
    return hip_ok(e, "bbdeheader reset", call_err_) ? 0 : -1;
}

} // namespace dvbs2
