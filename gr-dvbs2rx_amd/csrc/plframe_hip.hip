// plframe_hip.hip -- see plframe_hip.h. The estimate kernel runs ONE WAVEFRONT PER FRAME (a 64-thread workgroup): the
// PLSC is 64 symbols and the RM(64,7) transform has 64 points, so every step is one value per lane and every
// reduction a butterfly of cross-lane exchanges -- no LDS, no barrier. It reads 90 + 36 n_pilots symbols of a frame;
// the streaming payload step (plpayload_hip.hip) follows as a second launch on the same stream.
#include "plframe_hip.h"
#include "plsc_decode.hpp"
#include <cmath>
#include <vector>

namespace dvbs2 {

namespace {

using plsc::kPi;
using plsc::kS;
using plsc::remove_modulation;
using plsc::wave_sum;
using plsc::wrap_pi;

// the three data-aided sums over one PLHEADER (lib/pl_freq_sync.cc:201-226, :263-266); lane l holds symbols l and 64 + l
__device__ inline void header_sums(const float2* __restrict__ x, int l, uint64_t cw, float2* sof, float2* hdr, float2* last36)
{
    const int bit0 = plheader_bit(cw, l);
    const float2 t0 = remove_modulation(x[l], l, bit0);
    float2 t1 = make_float2(0.0f, 0.0f);
    if (l < 26) t1 = remove_modulation(x[64 + l], 64 + l, (int)((cw >> (25 - l)) & 1)); // plheader_bit(cw, 64 + l) without its SOF test
    const bool in_sof = l < 26, in_last = l >= 54;
    *sof = make_float2(wave_sum(in_sof ? t0.x : 0.0f), wave_sum(in_sof ? t0.y : 0.0f));
    *hdr = make_float2(wave_sum(t0.x + t1.x), wave_sum(t0.y + t1.y));
    *last36 = make_float2(wave_sum((in_last ? t0.x : 0.0f) + t1.x), wave_sum((in_last ? t0.y : 0.0f) + t1.y));
}

// one wavefront per frame; frame f starts at in + f * stride (plframe_len: back to back; more: a slot with its own next header)
__global__ __launch_bounds__(64) void pl_estimate_kernel(const float2* __restrict__ in, long long stride, const uint8_t* __restrict__ rn,
                                                         const uint8_t* __restrict__ rank, const int32_t* __restrict__ cc,
                                                         const float* __restrict__ cf, uint64_t hdr_cw, int plframe_len, int n_pilots,
                                                         int n_frames, int has_trailing, int coherent, int soft,
                                                         float* __restrict__ o_hph, float* __restrict__ o_inc, float* __restrict__ o_pil,
                                                         PlFrameEstimates est)
{
    const int f = blockIdx.x, l = threadIdx.x;
    const float2* __restrict__ x = in + (size_t)f * (size_t)stride;

    float2 sof, hdr, last36;
    header_sums(x, l, hdr_cw, &sof, &hdr, &last36);
    const float sof_phase = atan2f(sof.y, sof.x), hph = atan2f(hdr.y, hdr.x);

    // ---- PLSC of the frame's own header (lib/plsync_cc_impl.cc:582-590): de-rotate by the SOF phase
    // (lib/pl_freq_sync.cc:429-436), lane j takes PLSC symbol j = PLHEADER symbol 26 + j (plsc_decode.hpp)
    const int decoded = plsc::decode_wave(x[26 + l], x[25 + l], sof_phase, l, rank, coherent, soft);

    // ---- fine frequency offset
    const bool coarse = cc[f] != 0;
    float fine = 0.0f; int valid = 0;
    if (n_pilots > 0) {
        // lane 0: the last 36 PLHEADER symbols; lane i + 1: descrambled pilot block i (lib/pl_freq_sync.cc:263-273)
        float ar = last36.x, ai = last36.y;
        for (int i = 0; i < n_pilots; i++) {
            const int k = (i + 1) * 1476 - 36 + l; // payload offset
            float dr = 0.0f, di = 0.0f;
            if (l < 36) {
                const float2 p = x[90 + k];
                switch (rn[k]) { case 0: dr = p.x; di = p.y; break; case 1: dr = p.y; di = -p.x; break;
                                 case 2: dr = -p.x; di = -p.y; break; default: dr = -p.y; di = p.x; break; }
            }
            const float sr = wave_sum(dr), si = wave_sum(di);
            if (l == i + 1) { ar = sr; ai = si; }
        }
        float a = 0.0f;
        if (l <= n_pilots) {
            a = atan2f(ai, ar);
            if (l > 0) a = wrap_pi((float)((double)a - kPi / 4.0)); // the pilots sit at pi/4 (:243-249)
        }
        const float prev = __shfl_up(a, 1);
        const float d = (l >= 1 && l <= n_pilots) ? wrap_pi(a - prev) : 0.0f;
        const float sum_diff = wave_sum(d);
        if (coarse) { fine = (float)((double)sum_diff / (2.0 * kPi * 1476.0 * (double)n_pilots)); valid = 1; } // :299
        if (l >= 1 && l <= n_pilots) {
            o_pil[(size_t)f * n_pilots + l - 1] = a;
            if (est.pilot_phase) est.pilot_phase[(size_t)f * n_pilots + l - 1] = a;
        }
    } else if (coarse && (f + 1 < n_frames || has_trailing) && fabs((double)cf[f]) <= 1.0 / (2.0 * (double)plframe_len)) {
        // PLHEADER to PLHEADER (lib/pl_freq_sync.cc:325-343); the next header's phase is recomputed here with the same
        // arithmetic the next frame's own wavefront uses
        float2 s2, h2, l2;
        header_sums(x + plframe_len, l, hdr_cw, &s2, &h2, &l2);
        double delta = (double)(atan2f(h2.y, h2.x) - hph);
        if (delta > kPi) delta -= 2.0 * kPi; else if (delta < -kPi) delta += 2.0 * kPi;
        fine = (float)(delta / (2.0 * kPi * (double)plframe_len));
        valid = 1;
    }
    if (l == 0) {
        o_hph[f] = hph;
        o_inc[f] = coarse ? (float)(2.0 * kPi * (double)fine) : 0.0f; // lib/plsync_cc_impl.cc:725-726
        if (est.plsc_decoded) est.plsc_decoded[f] = (uint8_t)decoded;
        if (est.sof_phase) est.sof_phase[f] = sof_phase;
        if (est.plheader_phase) est.plheader_phase[f] = hph;
        if (est.fine_foffset) est.fine_foffset[f] = fine;
        if (est.fine_valid) est.fine_valid[f] = valid;
    }
}

} // namespace

PlFrameHip::PlFrameHip(int gold_code, int plsc, int max_frames, int device) : PlscListStage(device), max_frames_(max_frames)
{
    pls_ = pls_parse(plsc);
    pp_ = new (std::nothrow) PlPayloadHip(gold_code, pls_.n_slots, pls_.has_pilots, max_frames, device);
    if (!pp_) { err_.argument("out of memory"); return; } // (no argument, kArgument: notes/stage_error_codes.md)
    if (!pp_->ok()) { err_ = { pp_->error_code(), pp_->error() }; return; }
    DeviceGuard dev_guard(device_);
    const size_t npar = (size_t)max_frames_ * (2 + (pls_.n_pilots ? pls_.n_pilots : 1));
    if (!dev_guard.ok || alloc(&d_rank_, 128) != hipSuccess || alloc(&d_par_, npar) != hipSuccess) {
        err_.argument("device setup failed"); return; // (device failure, kArgument: notes/stage_error_codes.md)
    }
    if (set_expected_pls(nullptr, 0)) { err_.argument(call_err_.text); call_err_ = {}; } // (device failure, kArgument: notes/stage_error_codes.md)
}

PlFrameHip::~PlFrameHip() { delete pp_; }

int PlscListStage::set_expected_pls(const uint8_t* list, int n)
{
    Entry on(*this);
    uint8_t rank[128];
    if (!pls_rank_table(list, n, rank)) { call_err_.argument("codeword indexes must be within [0, 128)"); return -1; } // lib/reed_muller.cc:48-52
    if (!on.ok || hipMemcpy(d_rank_, rank, 128, hipMemcpyHostToDevice) != hipSuccess) { call_err_.device("copy of the codeword list failed"); return -1; }
    return 0;
}

int PlFrameHip::run_device(const float* d_plframes, int n_frames, int has_trailing_header, const int32_t* d_coarse_corrected,
                           const float* d_coarse_foffset, float* d_out, const PlFrameEstimates& est, hipStream_t stream)
{
    return launch(d_plframes, pls_.plframe_len, n_frames, has_trailing_header, d_coarse_corrected, d_coarse_foffset, d_out, est, stream);
}

int PlFrameHip::run_strided_device(const float* d_slots, int stride_syms, int n_frames, const int32_t* d_coarse_corrected,
                                   const float* d_coarse_foffset, float* d_out, const PlFrameEstimates& est, hipStream_t stream)
{
    if (stride_syms < pls_.plframe_len + 90) { call_err_.argument("stride below plframe_len + 90"); return -1; }
    return launch(d_slots, stride_syms, n_frames, 1, d_coarse_corrected, d_coarse_foffset, d_out, est, stream); // every slot has its next header
}

int PlFrameHip::launch(const float* d_plframes, int stride_syms, int n_frames, int has_trailing_header, const int32_t* d_coarse_corrected,
                       const float* d_coarse_foffset, float* d_out, const PlFrameEstimates& est, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames == 0) return 0;
    float* d_hph = d_par_; float* d_inc = d_par_ + max_frames_; float* d_pil = d_par_ + 2 * (size_t)max_frames_;
    hipLaunchKernelGGL(pl_estimate_kernel, dim3(n_frames), dim3(64), 0, stream, reinterpret_cast<const float2*>(d_plframes), (long long)stride_syms,
                       pp_->d_rn(), d_rank_, d_coarse_corrected, d_coarse_foffset, plsc_codeword(pls_.plsc) ^ kPlscScrambler, pls_.plframe_len,
                       pls_.n_pilots, n_frames, has_trailing_header ? 1 : 0, coherent_, soft_, d_hph, d_inc, d_pil, est);
    if (launched("pl estimate kernel launch")) return -1;
    if (!d_out) return 0;
    if (!pp_->process_device_strided(d_plframes, stride_syms, 90, n_frames, d_hph, d_inc, d_coarse_corrected, d_pil, d_out, stream)) return 0;
    call_err_ = { pp_->error_code(), pp_->error() }; // what the payload stage recorded
    return -1;
}

} // namespace dvbs2
