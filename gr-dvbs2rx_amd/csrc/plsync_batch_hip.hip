// plsync_batch_hip.hip -- see plsync_batch_hip.h. Every kernel here finds its stream's buffers and calls plsync_device.hpp.
#include "plsync_batch_hip.h"
#include "plsync_device.hpp"
#include <cstring>

namespace dvbs2 {

namespace {

using namespace plsync_dev;

// what a kernel needs to find stream s: the caller's rows and the handle's per-stream arrays
struct BatchView {
    const float2* x; long long stride;   // stream s starts at x + s * stride + call[s].first
    const PlSyncBatchCall* call;
    float* metric; long long metric_stride;
    float2* hist;                         // [s][2][89]
    PlSyncState* st;
    PlSyncBatchResult* res;
    PlSyncFrame* frames; long long max_frames;
};

// grid (tile, stream); a block beyond its stream's length leaves at once (the whole workgroup: the test is uniform)
__global__ __launch_bounds__(kThreads) void plsync_batch_metric_kernel(BatchView v)
{
    const int s = blockIdx.y;
    const long long tile0 = (long long)blockIdx.x * kTile;
    const PlSyncBatchCall c = v.call[s];
    if (tile0 >= c.n_syms) return;
    metric_tile(v.x + s * v.stride + c.first, c.n_syms, v.hist + ((size_t)s * 2 + v.st[s].hist_sel) * kHist, (int)tile0, v.metric + s * v.metric_stride);
}

// one wavefront per stream; a stream without symbols keeps its state and reports nothing
__global__ __launch_bounds__(64) void plsync_batch_track_kernel(BatchView v, const uint8_t* __restrict__ rank, TrackArgs a)
{
    const int s = blockIdx.x;
    const PlSyncBatchCall c = v.call[s];
    PlSyncBatchResult r = { 0, 0, 0, 0 };
    if (c.n_syms > 0) { // uniform
        const TrackResult t = track_wave(v.x + s * v.stride + c.first, c.n_syms, v.metric + s * v.metric_stride, v.hist + (size_t)s * 2 * kHist,
                                         v.st + s, rank, v.frames + s * v.max_frames, a);
        r.n_frames = t.n_frames; r.consumed = t.consumed; r.state = t.state; r.n_syms = c.n_syms;
    } else {
        r.state = v.st[s].state;
    }
    if (threadIdx.x == 0) v.res[s] = r;
}

__device__ inline bool batch_selects(const BatchView& v, int s, int i, int wanted, int len)
{
    return gather_selects(v.frames[s * v.max_frames + i], v.st[s].last_base, v.res[s].n_syms, wanted, len);
}

// ONE workgroup of 16 wavefronts: a wavefront counts the selected records of streams w, w + 16, ..., then one thread adds them up
__global__ __launch_bounds__(1024) void plsync_batch_count_kernel(BatchView v, int n_streams, int wanted, int32_t* __restrict__ offsets)
{
    __shared__ int cnt[kPlsyncBatchMaxStreams];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int len = pl_frame_shape(wanted).plframe_len;
    for (int s = w; s < n_streams; s += 16) {
        const int nrec = v.res[s].n_frames;
        int c = 0;
        for (int i = l; i < nrec; i += 64) c += batch_selects(v, s, i, wanted, len) ? 1 : 0;
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
        if (l == 0) cnt[s] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int s = 0; s < n_streams; s++) { offsets[s] = acc; acc += cnt[s]; }
        offsets[n_streams] = acc; // the true count, also above max_slots
    }
}

// grid (record, stream), one workgroup per record; a selected record counts the selected ones before it in its stream to find its slot
__global__ __launch_bounds__(256) void plsync_batch_gather_kernel(BatchView v, int wanted, const int32_t* __restrict__ offsets, float2* __restrict__ slots,
                                                                  int max_slots, int32_t* __restrict__ slot_record)
{
    __shared__ int cnt;
    const int f = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    if (f >= v.res[s].n_frames) return; // uniform, as every return below
    const int len = pl_frame_shape(wanted).plframe_len;
    if (!batch_selects(v, s, f, wanted, len)) return;
    if (t == 0) cnt = 0;
    __syncthreads();
    int before = 0;
    for (int i = t; i < f; i += 256) before += batch_selects(v, s, i, wanted, len) ? 1 : 0;
    if (before) atomicAdd(&cnt, before);
    __syncthreads();
    const int slot = offsets[s] + cnt;
    if (slot >= max_slots) return;
    // the frame and the 90 symbols behind it: gather_selects has seen that they lie inside the searched buffer
    const float2* __restrict__ src = v.x + s * v.stride + v.call[s].first + (v.frames[s * v.max_frames + f].sof_index - v.st[s].last_base);
    gather_copy(src, slots + (size_t)slot * (len + 90), len + 90, t);
    if (slot_record && t == 0) { slot_record[2 * (size_t)slot] = s; slot_record[2 * (size_t)slot + 1] = f; }
}

} // namespace

std::string plsync_batch_check(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames)
{
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return "plsc out of range (-1 = decode every header, 0..127)";
    if (unlock_thresh < 1 || unlock_thresh > 255) return "unlock_thresh out of range (1..255)";
    if (max_streams < 1 || max_streams > kPlsyncBatchMaxStreams) return "max_streams out of range (1..1024)";
    if (max_symbols < kPlsyncMinSymbols) return "max_symbols must be at least 33282 + 90";
    if (max_frames < 1 || max_frames > (1 << 20)) return "max_frames out of range (1..1048576)";
    return std::string();
}

PlSyncBatchHip::PlSyncBatchHip(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames, int device)
    : PlscListStage(device), fixed_plsc_(plsc_or_minus1), unlock_thresh_(unlock_thresh), max_streams_(max_streams), max_symbols_(max_symbols),
      max_frames_(max_frames)
{
    if (const std::string bad = plsync_batch_check(plsc_or_minus1, unlock_thresh, max_streams, max_symbols, max_frames); !bad.empty()) { err_.argument(bad); return; }
    DeviceGuard dev_guard(device_);
    const size_t ns = (size_t)max_streams_;
    if (!dev_guard.ok || alloc(&d_rank_, 128) != hipSuccess || alloc(&d_metric_, ns * (size_t)max_symbols_) != hipSuccess ||
        alloc(&d_hist_, ns * 2 * kHist) != hipSuccess || alloc(&d_state_, ns) != hipSuccess || alloc(&d_call_, ns) != hipSuccess ||
        alloc(&d_res_, ns) != hipSuccess) {
        err_.argument("device setup failed"); return; // (device failure, kArgument: notes/stage_error_codes.md)
    }
    call_.resize(ns);
    res_.resize(ns);
    if (set_expected_pls(nullptr, 0) || reset()) { err_.argument(call_err_.text); call_err_ = {}; } // (device failure, kArgument: notes/stage_error_codes.md)
}

// streams first_stream .. first_stream + count as created: PlSyncHip::reset for each, and nothing of a last search
int PlSyncBatchHip::write_fresh(int first_stream, int count)
{
    Entry on(*this);
    PlSyncState s;
    std::memset(&s, 0, sizeof(s));
    s.abs_last_peak = -1; // d_sym_cnt = 0 before the first symbol (lib/pl_frame_sync.cc:23)
    s.frame_len = fixed_plsc_ >= 0 ? pl_frame_shape(fixed_plsc_).plframe_len : 0; // lib/plsync_cc_impl.cc:159, lib/pl_frame_sync.cc:28
    const std::vector<PlSyncState> all((size_t)count, s);
    // a search that is still pending on the caller's stream writes the states and the histories behind itself: wait for it first (the
    // null stream of the copies below does not order itself against a non-blocking stream)
    if (!on.ok || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(d_state_ + first_stream, all.data(), all.size() * sizeof(PlSyncState), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_hist_ + (size_t)first_stream * 2 * kHist, 0, (size_t)count * 2 * kHist * sizeof(float2)) != hipSuccess ||
        hipMemset(d_call_ + first_stream, 0, (size_t)count * sizeof(PlSyncBatchCall)) != hipSuccess ||
        memset_done(d_res_ + first_stream, 0, (size_t)count * sizeof(PlSyncBatchResult)) != hipSuccess) {
        call_err_.device("reset of the device state failed"); return -1;
    }
    return 0;
}

int PlSyncBatchHip::reset() { return write_fresh(0, max_streams_); }

int PlSyncBatchHip::reset_stream(int s)
{
    if (s < 0 || s >= max_streams_) { call_err_.argument("stream index out of range"); return -1; }
    return write_fresh(s, 1);
}

int PlSyncBatchHip::search_device(const float* d_syms, int64_t stride_syms, const int* first, const int* n_syms, int n_streams, PlSyncFrame* d_frames,
                                  hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_streams < 0 || n_streams > max_streams_) { call_err_.device("n_streams exceeds max_streams"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    int max_n = 0;
    for (int s = 0; s < n_streams; s++) {
        if (first[s] < 0 || n_syms[s] < 0 || n_syms[s] > max_symbols_) { call_err_.device("n_syms exceeds max_symbols"); return -1; } // (the same)
        call_[s] = { first[s], n_syms[s] };
        if (n_syms[s] > max_n) max_n = n_syms[s];
    }
    last_streams_ = n_streams; last_max_n_ = max_n; last_stream_ = stream;
    if (n_streams == 0) return 0;
    if (hipMemcpyAsync(d_call_, call_.data(), (size_t)n_streams * sizeof(PlSyncBatchCall), hipMemcpyHostToDevice, stream) != hipSuccess) {
        call_err_.device("copy of the symbol counts failed"); return -1;
    }
    const BatchView v = { reinterpret_cast<const float2*>(d_syms), (long long)stride_syms, d_call_, d_metric_, (long long)max_symbols_, d_hist_, d_state_,
                          d_res_, d_frames, (long long)max_frames_ };
    if (max_n > 0) {
        hipLaunchKernelGGL(plsync_batch_metric_kernel, dim3((max_n + kTile - 1) / kTile, n_streams), dim3(kThreads), 0, stream, v);
        if (launched("plsync batch metric kernel launch")) return -1;
    }
    hipLaunchKernelGGL(plsync_batch_track_kernel, dim3(n_streams), dim3(64), 0, stream, v, d_rank_,
                       TrackArgs{ max_frames_, fixed_plsc_, unlock_thresh_, coherent_, soft_ });
    return launched("plsync batch tracker kernel launch");
}

int PlSyncBatchHip::finish(int* n_frames, int* consumed, int* state)
{
    Entry on(*this);
    if (!on.ok || hipStreamSynchronize(last_stream_) != hipSuccess ||
        (last_streams_ && hipMemcpy(res_.data(), d_res_, (size_t)last_streams_ * sizeof(PlSyncBatchResult), hipMemcpyDeviceToHost) != hipSuccess)) {
        call_err_.device("reading the results failed"); return -1;
    }
    for (int s = 0; s < last_streams_; s++) {
        if (n_frames) n_frames[s] = res_[s].n_frames;
        if (consumed) consumed[s] = res_[s].consumed;
        if (state) state[s] = res_[s].state;
    }
    return last_streams_;
}

int PlSyncBatchHip::gather_device(const float* d_syms, int64_t stride_syms, const PlSyncFrame* d_frames, int n_streams, int wanted_plsc, float* d_slots,
                                  int max_slots, int32_t* d_offsets, int32_t* d_slot_record, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_streams < 0 || n_streams > last_streams_) { call_err_.argument("n_streams exceeds the streams of the last search"); return -1; }
    if (n_streams == 0) {
        if (hipMemsetAsync(d_offsets, 0, sizeof(int32_t), stream) != hipSuccess) { call_err_.device("clearing the slot count failed"); return -1; }
        return 0;
    }
    const BatchView v = { reinterpret_cast<const float2*>(d_syms), (long long)stride_syms, d_call_, d_metric_, (long long)max_symbols_, d_hist_, d_state_,
                          d_res_, const_cast<PlSyncFrame*>(d_frames), (long long)max_frames_ };
    hipLaunchKernelGGL(plsync_batch_count_kernel, dim3(1), dim3(1024), 0, stream, v, n_streams, wanted_plsc, d_offsets);
    if (launched("plsync batch count kernel launch")) return -1;
    const int max_rec = last_max_n_ < max_frames_ ? last_max_n_ : max_frames_; // no stream of the last search reported more records
    if (max_rec == 0 || max_slots == 0) return 0;
    hipLaunchKernelGGL(plsync_batch_gather_kernel, dim3(max_rec, n_streams), dim3(256), 0, stream, v, wanted_plsc, d_offsets,
                       reinterpret_cast<float2*>(d_slots), max_slots, d_slot_record);
    return launched("plsync batch gather kernel launch");
}

} // namespace dvbs2
