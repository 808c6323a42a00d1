// plsync_hip.hip -- see plsync_hip.h. The device code is in plsync_device.hpp, which the batched stage (plsync_batch_hip.hip) shares:
// the kernels here are one stream's view of it.
#include "plsync_device.hpp"
#include <cmath>
#include <cstring>

namespace dvbs2 {

namespace {

using namespace plsync_dev;

__global__ __launch_bounds__(kThreads) void plsync_metric_kernel(const float2* __restrict__ x, int n_syms, const float2* __restrict__ hist2,
                                                                 const PlSyncState* __restrict__ st, float* __restrict__ metric)
{
    metric_tile(x, n_syms, hist2 + st->hist_sel * kHist, blockIdx.x * kTile, metric);
}

// one wavefront
__global__ __launch_bounds__(64) void plsync_track_kernel(const float2* __restrict__ x, int n_syms, const float* __restrict__ metric,
                                                          float2* __restrict__ hist2, PlSyncState* __restrict__ st,
                                                          const uint8_t* __restrict__ rank, PlSyncFrame* __restrict__ frames, TrackArgs a)
{
    track_wave(x, n_syms, metric, hist2, st, rank, frames, a);
}

// one workgroup per record; a selected record counts the selected ones before and after it to find its slot
__global__ __launch_bounds__(256) void plsync_gather_kernel(const float2* __restrict__ x, const PlSyncFrame* __restrict__ frames, int n_frames,
                                                            const PlSyncState* __restrict__ st, int wanted, float2* __restrict__ out,
                                                            int32_t* __restrict__ count)
{
    __shared__ int cnt[2];
    const int f = blockIdx.x, t = threadIdx.x;
    const int nrec = n_frames < st->last_n_frames ? n_frames : st->last_n_frames, n_syms = st->last_n_syms;
    const int64_t base = st->last_base;
    const int len = pl_frame_shape(wanted).plframe_len;
    auto selected = [&](int i) { return i < nrec && gather_selects(frames[i], base, n_syms, wanted, len); };
    const bool mine = selected(f);
    if (!mine && f != 0) return; // only a selected record needs its slot; block 0 stays to write a count of 0 when nothing is selected
    if (t < 2) cnt[t] = 0;
    __syncthreads();
    int before = 0, after = 0;
    for (int i = t; i < nrec; i += 256) { if (selected(i)) { if (i < f) before++; else if (i > f) after++; } }
    if (before) atomicAdd(&cnt[0], before);
    if (after) atomicAdd(&cnt[1], after);
    __syncthreads();
    before = cnt[0]; after = cnt[1];
    if (f == 0 && t == 0 && !mine && after == 0) *count = 0;
    if (!mine) return;
    const int n = after == 0 ? len + 90 : len; // the last one takes the header after it along
    gather_copy(x + (frames[f].sof_index - base), out + (size_t)before * len, n, t);
    if (after == 0 && t == 0) *count = before + 1;
}

} // namespace

PlSyncHip::PlSyncHip(int plsc_or_minus1, int unlock_thresh, int max_symbols, int max_frames, int device)
    : PlscListStage(device), fixed_plsc_(plsc_or_minus1), unlock_thresh_(unlock_thresh), max_symbols_(max_symbols), max_frames_(max_frames)
{
    // the compile-time tap signs against the expected symbols
    float sof[25], pl[32];
    plsync_taps(sof, pl);
    for (int k = 1; k <= 25; k++) if ((sof[k - 1] < 0.0f) != tap_minus(k)) { err_.argument("SOF tap signs disagree with the PLHEADER"); return; }
    for (int i = 0; i < 32; i++) if ((pl[i] < 0.0f) != tap_minus(27 + 2 * i)) { err_.argument("PLSC tap signs disagree with the PLHEADER"); return; }
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok || alloc(&d_rank_, 128) != hipSuccess || alloc(&d_metric_, (size_t)max_symbols_) != hipSuccess ||
        alloc(&d_hist_, 2 * kHist) != hipSuccess || alloc(&d_state_, 1) != hipSuccess) {
        err_.argument("device setup failed"); return; // (device failure, kArgument: notes/stage_error_codes.md)
    }
    if (set_expected_pls(nullptr, 0) || reset()) { err_.argument(call_err_.text); call_err_ = {}; } // (device failure, kArgument: notes/stage_error_codes.md)
}

int PlSyncHip::reset()
{
    Entry on(*this);
    PlSyncState s;
    std::memset(&s, 0, sizeof(s));
    s.abs_last_peak = -1; // d_sym_cnt = 0 before the first symbol (lib/pl_frame_sync.cc:23)
    s.frame_len = fixed_plsc_ >= 0 ? pl_frame_shape(fixed_plsc_).plframe_len : 0; // lib/plsync_cc_impl.cc:159, lib/pl_frame_sync.cc:28
    // a search that is still pending on the caller's stream writes the state and the history behind itself: wait for it first (the
    // null stream of the two copies below does not order itself against a non-blocking stream)
    if (!on.ok || hipDeviceSynchronize() != hipSuccess || hipMemcpy(d_state_, &s, sizeof(s), hipMemcpyHostToDevice) != hipSuccess ||
        memset_done(d_hist_, 0, 2 * kHist * sizeof(float2)) != hipSuccess) { call_err_.device("reset of the device state failed"); return -1; }
    return 0;
}

int PlSyncHip::metric_device(const float* d_syms, int n_syms, float* d_metric, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_syms <= 0) return 0;
    hipLaunchKernelGGL(plsync_metric_kernel, dim3((n_syms + kTile - 1) / kTile), dim3(kThreads), 0, stream,
                       reinterpret_cast<const float2*>(d_syms), n_syms, d_hist_, d_state_, d_metric);
    return launched("plsync metric kernel launch");
}

int PlSyncHip::search_device(const float* d_syms, int n_syms, PlSyncFrame* d_frames, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_syms < 0 || n_syms > max_symbols_) { call_err_.device("n_syms exceeds max_symbols"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (metric_device(d_syms, n_syms, d_metric_, stream)) return -1;
    hipLaunchKernelGGL(plsync_track_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const float2*>(d_syms), n_syms, d_metric_, d_hist_,
                       d_state_, d_rank_, d_frames, TrackArgs{ max_frames_, fixed_plsc_, unlock_thresh_, coherent_, soft_ });
    if (launched("plsync tracker kernel launch")) return -1;
    last_stream_ = stream;
    return 0;
}

int PlSyncHip::finish(int* n_frames, int* consumed, int* state)
{
    Entry on(*this);
    PlSyncState s;
    if (!on.ok || hipStreamSynchronize(last_stream_) != hipSuccess ||
        hipMemcpy(&s, d_state_, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) { call_err_.device("reading the device state failed"); return -1; }
    if (n_frames) *n_frames = s.last_n_frames;
    if (consumed) *consumed = s.last_consumed;
    if (state) *state = s.state;
    return 0;
}

int PlSyncHip::gather_device(const float* d_syms, const PlSyncFrame* d_frames, int n_frames, int wanted_plsc, float* d_plframes,
                             int32_t* d_count, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames == 0) {
        if (hipMemsetAsync(d_count, 0, sizeof(int32_t), stream) != hipSuccess) { call_err_.device("clearing the frame count failed"); return -1; }
        return 0;
    }
    hipLaunchKernelGGL(plsync_gather_kernel, dim3(n_frames), dim3(256), 0, stream, reinterpret_cast<const float2*>(d_syms), d_frames, n_frames,
                       d_state_, wanted_plsc, reinterpret_cast<float2*>(d_plframes), d_count);
    return launched("plsync gather kernel launch");
}

} // namespace dvbs2
