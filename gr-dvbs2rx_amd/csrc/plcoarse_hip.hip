// plcoarse_hip.hip -- see plcoarse_hip.h.
#include "plcoarse_hip.h"
#include "plsc_decode.hpp"
#include <cmath>
#include <cstring>
#include <new>

namespace dvbs2 {

namespace {

using plsc::kPi;
using plsc::unmod;
using plsc::wave_sum;
using plsc::wrap_pi;
constexpr int kBatch = 16; // frames the window kernel loads ahead of the serial walk

// One pass over a header of N symbols held as z0 (symbols 0..63 in lanes 0..63) and z1 (symbols 64..N-1 in lanes 0..N-65): lane l
// leaves lag l in *a (sum over u = 0 .. N-l-1 of z[u+l] conj(z[u]), ascending u) and lag N - l in *b (u = N-l .. N-1 of
// z[u] conj(z[u+l-N]), ascending u). All 64 lanes take part in every exchange.
template <int N> __device__ inline void lag_pair(float2 z0, float2 z1, int l, float2* a, float2* b)
{
    float2 sa = make_float2(0.0f, 0.0f), sb = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int u = 0; u < N; u++) {
        const float2 zu = u < 64 ? make_float2(__shfl(z0.x, u), __shfl(z0.y, u)) : make_float2(__shfl(z1.x, u - 64), __shfl(z1.y, u - 64));
        int idx = u + l;
        const bool wrapped = idx >= N;
        if (wrapped) idx -= N;
        const int src = idx & 63;
        float2 zo = make_float2(__shfl(z0.x, src), __shfl(z0.y, src));
        if (N > 64) {
            const float2 hi = make_float2(__shfl(z1.x, src), __shfl(z1.y, src));
            if (idx >= 64) zo = hi;
        }
        const float re = zo.x * zu.x + zo.y * zu.y, im = zo.y * zu.x - zo.x * zu.y; // zo conj(zu)
        if (!wrapped) { sa.x += re; sa.y += im; } else { sb.x += re; sb.y -= im; }  // after the wrap the pair is zu conj(zo)
    }
    *a = sa; *b = sb;
}

// one wavefront per header; r: kPlcoarseRecord float2 per frame, [0].x = 1 when the record holds a frame. total (nullable): the number
// of frames there really are, on the device; a wavefront at or beyond it leaves at once
__global__ __launch_bounds__(64) void plcoarse_autocorr_kernel(const float2* __restrict__ x, long long stride, const uint8_t* __restrict__ plsc,
                                                               int fixed_plsc, const PlSyncFrame* __restrict__ rec, int n_syms, long long base,
                                                               const uint64_t* __restrict__ cwtab, float2* __restrict__ r,
                                                               const int32_t* __restrict__ total)
{
    const int f = blockIdx.x, l = threadIdx.x;
    if (total && f >= *total) return;
    float2* __restrict__ R = r + (size_t)f * kPlcoarseRecord;
    const float2* __restrict__ h;
    int p;
    if (rec) {
        const PlSyncFrame q = rec[f];
        const long long rel = q.sof_index - base;
        if (rel < 0 || rel + 90 > (long long)n_syms) { if (l == 0) R[0] = make_float2(0.0f, 0.0f); return; } // the whole wavefront leaves
        h = x + rel; p = q.plsc & 127;
    } else {
        h = x + (long long)f * stride; p = plsc ? (plsc[f] & 127) : fixed_plsc;
    }
    const uint64_t cw = cwtab[p];
    const int bit0 = plheader_bit(cw, l);
    const float2 z0 = unmod(h[l], l, bit0);
    float2 z1 = make_float2(0.0f, 0.0f);
    if (l < 26) z1 = unmod(h[64 + l], 64 + l, (int)((cw >> (25 - l)) & 1)); // plheader_bit(cw, 64 + l) without its SOF test

    float2 a, b;
    lag_pair<90>(z0, z1, l, &a, &b);
    if (l >= 1 && l <= 45) R[l] = a;
    if (l >= 1 && l <= 44) R[90 - l] = b; // lane 45's second half is lag 45 again: the same pairs, not written
    lag_pair<26>(z0, z1, l, &a, &b);
    if (l >= 1 && l <= 13) R[90 + l] = a;
    if (l >= 1 && l <= 12) R[90 + 26 - l] = b;
    if (l == 0) { R[0] = make_float2(1.0f, 0.0f); R[90] = make_float2(0.0f, 0.0f); }
}

// one wavefront walks n_frames records in order over one state; lane l holds lags l + 1 and l + 65
__device__ inline void window_walk(const float2* __restrict__ r, int n_frames, int period, int always_full, const float* __restrict__ w,
                                   PlCoarseState* __restrict__ st, PlCoarseOut out)
{
    const int l = threadIdx.x;
    const bool hi = l < 25; // the lane has a second lag (full form) / a lag at all (SOF form)
    float2 a0 = st->acc[l + 1], a1 = hi ? st->acc[l + 65] : make_float2(0.0f, 0.0f);
    int i_frame = st->i_frame, corrected = st->corrected;
    float fo = st->foffset;
    const float wf0 = w[l], wf1 = hi ? w[64 + l] : 0.0f, ws0 = hi ? w[89 + l] : 0.0f;

    for (int f0 = 0; f0 < n_frames; f0 += kBatch) {
        float2 v0[kBatch], v1[kBatch], vs[kBatch];
        float valid[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++) { // the loads do not depend on the state: all in flight before the serial part
            const int f = f0 + i < n_frames ? f0 + i : n_frames - 1;
            const float2* __restrict__ R = r + (size_t)f * kPlcoarseRecord;
            valid[i] = R[0].x;
            v0[i] = R[l + 1];
            v1[i] = hi ? R[l + 65] : make_float2(0.0f, 0.0f);
            vs[i] = hi ? R[90 + l + 1] : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            const int f = f0 + i;
            int new_est = 0;
            if (f < n_frames && valid[i] != 0.0f) { // uniform over the wavefront
                const bool full = always_full || corrected; // lib/plsync_cc_impl.cc:567-569
                if (full) { a0.x += v0[i].x; a0.y += v0[i].y; a1.x += v1[i].x; a1.y += v1[i].y; }
                else { a0.x += vs[i].x; a0.y += vs[i].y; }
                if (++i_frame >= period) {
                    const int L = full ? 89 : 25;
                    const bool on0 = l + 1 <= L, on1 = full && hi;
                    const float th0 = on0 ? atan2f(a0.y, a0.x) : 0.0f, th1 = on1 ? atan2f(a1.y, a1.x) : 0.0f;
                    float p0 = __shfl_up(th0, 1), p1 = __shfl_up(th1, 1);
                    const float th64 = __shfl(th0, 63);
                    if (l == 0) { p0 = 0.0f; p1 = th64; } // angle_corr[0] = 0; lag 65 follows lag 64
                    const float d0 = on0 ? wrap_pi(th0 - p0) : 0.0f, d1 = on1 ? wrap_pi(th1 - p1) : 0.0f;
                    const float t0 = (full ? wf0 : ws0) * d0, t1 = wf1 * d1;
                    const float s = wave_sum(t0 + t1);
                    float e = (float)((double)s / (2.0 * kPi));
                    e = e > 0.5f ? 0.5f : (e < -0.5f ? -0.5f : e);
                    fo = e;
                    corrected = fabs((double)e) < kFineFoffsetCorrRange ? 1 : 0;
                    a0 = make_float2(0.0f, 0.0f); a1 = make_float2(0.0f, 0.0f);
                    i_frame = 0; new_est = 1;
                }
            }
            if (l == 0 && f < n_frames) {
                if (out.foffset) out.foffset[f] = fo;
                if (out.corrected) out.corrected[f] = corrected;
                if (out.new_est) out.new_est[f] = new_est;
            }
        }
    }
    st->acc[l + 1] = a0;
    if (hi) st->acc[l + 65] = a1;
    if (l == 0) { st->i_frame = i_frame; st->corrected = corrected; st->foffset = fo; }
}

__global__ __launch_bounds__(64) void plcoarse_window_kernel(const float2* __restrict__ r, int n_frames, int period, int always_full,
                                                             const float* __restrict__ w, PlCoarseState* __restrict__ st, PlCoarseOut out)
{
    window_walk(r, n_frames, period, always_full, w, st, out);
}

// one wavefront per stream: stream s walks slots offsets[s] .. offsets[s + 1] (below max_slots) over its own state
__global__ __launch_bounds__(64) void plcoarse_batch_window_kernel(const float2* __restrict__ r, const int32_t* __restrict__ offsets, int max_slots,
                                                                   int period, int always_full, const float* __restrict__ w,
                                                                   PlCoarseState* __restrict__ st, PlCoarseOut out)
{
    const int s = blockIdx.x;
    const int a = offsets[s] < max_slots ? offsets[s] : max_slots, b = offsets[s + 1] < max_slots ? offsets[s + 1] : max_slots;
    if (b <= a) return; // uniform: the stream has no slot in this call, its state stays
    PlCoarseOut o;
    o.foffset = out.foffset ? out.foffset + a : nullptr;
    o.corrected = out.corrected ? out.corrected + a : nullptr;
    o.new_est = out.new_est ? out.new_est + a : nullptr;
    window_walk(r + (size_t)a * kPlcoarseRecord, b - a, period, always_full, w, st + s, o);
}

} // namespace

PlCoarseHip::PlCoarseHip(int period, int plsc_or_minus1, int max_frames, int device)
    : DeviceStage(device), period_(period), fixed_plsc_(plsc_or_minus1), max_frames_(max_frames)
{
    uint64_t cw[128];
    for (int p = 0; p < 128; p++) cw[p] = plsc_codeword(p) ^ kPlscScrambler;
    float w[89 + 25];
    plcoarse_weights(1, w); plcoarse_weights(0, w + 89);
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok || alloc(&d_cw_, 128) != hipSuccess || alloc(&d_w_, 89 + 25) != hipSuccess ||
        alloc(&d_r_, (size_t)max_frames_ * kPlcoarseRecord) != hipSuccess || alloc(&d_state_, 1) != hipSuccess ||
        hipMemcpy(d_cw_, cw, sizeof(cw), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_w_, w, sizeof(w), hipMemcpyHostToDevice) != hipSuccess) {
        err_.argument("device setup failed"); return; // (device failure, kArgument: notes/stage_error_codes.md)
    }
    if (reset()) { err_.argument(call_err_.text); call_err_ = {}; } // (device failure, kArgument: notes/stage_error_codes.md)
}

int PlCoarseHip::reset()
{
    Entry on(*this);
    // all zero: no frame counted, empty accumulator, estimate 0, not coarse-corrected (lib/pl_freq_sync.cc:24-31)
    if (!on.ok || hipDeviceSynchronize() != hipSuccess || memset_done(d_state_, 0, sizeof(PlCoarseState)) != hipSuccess) {
        call_err_.device("reset of the device state failed"); return -1;
    }
    return 0;
}

int PlCoarseHip::launch(const float2* x, int64_t stride, const uint8_t* plsc, const PlSyncFrame* rec, int n_syms, int64_t base, int n_frames,
                        const PlCoarseOut& out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames == 0) return 0;
    hipLaunchKernelGGL(plcoarse_autocorr_kernel, dim3(n_frames), dim3(64), 0, stream, x, (long long)stride, plsc, fixed_plsc_ < 0 ? 0 : fixed_plsc_,
                       rec, n_syms, (long long)base, d_cw_, d_r_, nullptr);
    if (launched("plcoarse autocorrelation kernel launch")) return -1;
    hipLaunchKernelGGL(plcoarse_window_kernel, dim3(1), dim3(64), 0, stream, d_r_, n_frames, period_, fixed_plsc_ >= 0 ? 1 : 0, d_w_, d_state_, out);
    return launched("plcoarse window kernel launch");
}

int PlCoarseHip::frames_device(const float* d_plframes, int64_t stride_syms, const uint8_t* d_plsc, int n_frames, const PlCoarseOut& out,
                               hipStream_t stream)
{
    return launch(reinterpret_cast<const float2*>(d_plframes), stride_syms, d_plsc, nullptr, 0, 0, n_frames, out, stream);
}

int PlCoarseHip::records_device(const float* d_syms, int n_syms, const PlSyncFrame* d_records, int n_frames, int64_t base, const PlCoarseOut& out,
                                hipStream_t stream)
{
    return launch(reinterpret_cast<const float2*>(d_syms), 0, nullptr, d_records, n_syms, base, n_frames, out, stream);
}

} // namespace dvbs2

namespace dvbs2 {

std::string plcoarse_batch_check(int period, int plsc_or_minus1, int max_streams, int max_slots)
{
    if (period < 1) return "period must be at least 1";
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return "plsc out of range (-1 = not known, 0..127)";
    if (max_streams < 1 || max_streams > kPlsyncBatchMaxStreams) return "max_streams out of range (1..1024)";
    if (max_slots < 1 || max_slots > (1 << 20)) return "max_slots out of range (1..1048576)";
    return std::string();
}

PlCoarseBatchHip::PlCoarseBatchHip(int period, int plsc_or_minus1, int max_streams, int max_slots, int device)
    : DeviceStage(device), period_(period), fixed_plsc_(plsc_or_minus1), max_streams_(max_streams), max_slots_(max_slots)
{
    if (const std::string bad = plcoarse_batch_check(period, plsc_or_minus1, max_streams, max_slots); !bad.empty()) { err_.argument(bad); return; }
    uint64_t cw[128];
    for (int p = 0; p < 128; p++) cw[p] = plsc_codeword(p) ^ kPlscScrambler;
    float w[89 + 25];
    plcoarse_weights(1, w); plcoarse_weights(0, w + 89);
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok || alloc(&d_cw_, 128) != hipSuccess || alloc(&d_w_, 89 + 25) != hipSuccess ||
        alloc(&d_r_, (size_t)max_slots_ * kPlcoarseRecord) != hipSuccess || alloc(&d_state_, (size_t)max_streams_) != hipSuccess ||
        hipMemcpy(d_cw_, cw, sizeof(cw), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_w_, w, sizeof(w), hipMemcpyHostToDevice) != hipSuccess) {
        err_.argument("device setup failed"); return; // (device failure, kArgument: notes/stage_error_codes.md)
    }
    if (reset()) { err_.argument(call_err_.text); call_err_ = {}; } // (device failure, kArgument: notes/stage_error_codes.md)
}

int PlCoarseBatchHip::clear(int first_stream, int count)
{
    Entry on(*this);
    // all zero, as PlCoarseHip::reset, for these streams only
    if (!on.ok || hipDeviceSynchronize() != hipSuccess || memset_done(d_state_ + first_stream, 0, (size_t)count * sizeof(PlCoarseState)) != hipSuccess) {
        call_err_.device("reset of the device state failed"); return -1;
    }
    return 0;
}

int PlCoarseBatchHip::reset() { return clear(0, max_streams_); }

int PlCoarseBatchHip::reset_stream(int s)
{
    if (s < 0 || s >= max_streams_) { call_err_.argument("stream index out of range"); return -1; }
    return clear(s, 1);
}

int PlCoarseBatchHip::slots_device(const float* d_slots, int64_t stride_syms, const uint8_t* d_plsc, const int32_t* d_offsets, int n_streams,
                                   const PlCoarseOut& out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_streams < 0 || n_streams > max_streams_) { call_err_.device("n_streams exceeds max_streams"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_streams == 0) return 0;
    // over max_slots: the count is on the device, wavefronts at or beyond d_offsets[n_streams] leave at once
    hipLaunchKernelGGL(plcoarse_autocorr_kernel, dim3(max_slots_), dim3(64), 0, stream, reinterpret_cast<const float2*>(d_slots), (long long)stride_syms, d_plsc,
                       fixed_plsc_ < 0 ? 0 : fixed_plsc_, nullptr, 0, 0ll, d_cw_, d_r_, d_offsets + n_streams);
    if (launched("plcoarse autocorrelation kernel launch")) return -1;
    hipLaunchKernelGGL(plcoarse_batch_window_kernel, dim3(n_streams), dim3(64), 0, stream, d_r_, d_offsets, max_slots_, period_, fixed_plsc_ >= 0 ? 1 : 0,
                       d_w_, d_state_, out);
    return launched("plcoarse batch window kernel launch");
}

} // namespace dvbs2
