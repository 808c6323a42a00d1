// plpayload_hip.hip -- see plpayload_hip.h. Streaming kernel, HBM bound: 8 B in + 8 B out per data symbol.
#include "plpayload_hip.h"
#include <cmath>

namespace dvbs2 {

// one thread per output (data) symbol; grid.y = frame. Frame f's payload starts at in[f * frame_stride + in_offset]:
// (payload_len, 0) for payloads back to back, (plframe_len, 90) for whole PLFRAMEs (plframe_hip.hip)
__global__ void pl_payload_kernel(const float2* __restrict__ in, const uint8_t* __restrict__ rn, const float* __restrict__ hphase,
                                  const float* __restrict__ pinc, const int32_t* __restrict__ cc, const float* __restrict__ pphase,
                                  float2* __restrict__ out, int n_slots, int n_pilots, int has_pilots, int frame_stride, int in_offset)
{
    const int f = blockIdx.y;
    const int n_out = n_slots * 90;
    const bool coarse = cc[f] != 0;
    const double inc = coarse ? (double)pinc[f] : 0.0;
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += gridDim.x * blockDim.x) {
        const int slot = o / 90;
        const int blk = has_pilots ? slot / 16 : 0;
        const int k = o + blk * 36; // index in the payload: pilot blocks are skipped (lib/plsync_cc_impl.cc:480-485)
        // rotator state: reset to the preceding pilot block's phase at every 16-slot segment of a coarse-corrected
        // frame (:759-763); otherwise it runs on from the PLHEADER phase (:652)
        double theta0; int steps;
        if (coarse && blk > 0) { theta0 = (double)pphase[(size_t)f * n_pilots + blk - 1]; steps = o - blk * 16 * 90; }
        else { theta0 = (double)hphase[f]; steps = o; }
        double s, c;
        sincos(-(theta0 + inc * (double)steps), &s, &c);
        const float2 x = in[(size_t)f * frame_stride + in_offset + k];
        float dr, di; // descrambling: multiply by conj(exp(j Rn pi/2)) in {1, -j, -1, j} (lib/pl_descrambler.cc:56-58); the same
                      // statement stands in pl_estimate_kernel (plframe_hip.hip), see plsc_decode.hpp for why it is no function
        switch (rn[k]) { case 0: dr = x.x; di = x.y; break; case 1: dr = x.y; di = -x.x; break;
                         case 2: dr = -x.x; di = -x.y; break; default: dr = -x.y; di = x.x; break; }
        const float pr = (float)c, pi = (float)s;
        out[(size_t)f * n_out + o] = make_float2(dr * pr - di * pi, dr * pi + di * pr);
    }
}

PlPayloadHip::PlPayloadHip(int gold_code, int n_slots, int has_pilots, int max_frames, int device)
    : DeviceStage(device), n_slots_(n_slots), has_pilots_(has_pilots ? 1 : 0), max_frames_(max_frames)
{
    n_pilots_ = pl_pilot_blocks(n_slots_, has_pilots_);
    if (n_slots_ < 36 || n_slots_ > 360) { err_.argument("n_slots out of range (36..360)"); return; } // lib/pl_defs.h:19-20
    if (gold_code < 0 || gold_code >= (1 << 18) - 1) { err_.argument("gold code out of range"); return; }
    if (max_frames_ < 1 || max_frames_ > 65535) { err_.argument("max_frames must be in 1..65535 (frames are one launch dimension)"); return; }
    std::vector<uint8_t> rn(payload_len());
    pl_scrambling_rn(gold_code, rn.data(), (int)rn.size());
    DeviceGuard dev_guard(device_); // the caller's current device is restored on return
    if (!dev_guard.ok || alloc(&d_rn_, rn.size()) != hipSuccess ||
        hipMemcpy(d_rn_, rn.data(), rn.size(), hipMemcpyHostToDevice) != hipSuccess) { err_.argument("device setup failed"); return; } // (device failure, kArgument: notes/stage_error_codes.md)
}

int PlPayloadHip::process_device(const float* d_payload, int n_frames, const float* d_plheader_phase, const float* d_phase_inc,
                                 const int32_t* d_coarse_corrected, const float* d_pilot_phase, float* d_out, hipStream_t stream)
{
    return process_device_strided(d_payload, payload_len(), 0, n_frames, d_plheader_phase, d_phase_inc, d_coarse_corrected, d_pilot_phase,
                                  d_out, stream);
}

int PlPayloadHip::process_device_strided(const float* d_in, int frame_stride, int in_offset, int n_frames, const float* d_plheader_phase,
                                         const float* d_phase_inc, const int32_t* d_coarse_corrected, const float* d_pilot_phase,
                                         float* d_out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames == 0) return 0;
    hipLaunchKernelGGL(pl_payload_kernel, dim3((xfecframe_len() + 255) / 256, n_frames), dim3(256), 0, stream,
                       reinterpret_cast<const float2*>(d_in), d_rn_, d_plheader_phase, d_phase_inc, d_coarse_corrected,
                       d_pilot_phase, reinterpret_cast<float2*>(d_out), n_slots_, n_pilots_, has_pilots_, frame_stride, in_offset);
    return launched("pl payload kernel launch");
}

} // namespace dvbs2
