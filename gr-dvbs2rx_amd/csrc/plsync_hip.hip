// plsync_hip.hip -- see plsync_hip.h.
// Metric kernel: a workgroup of 256 threads owns a tile of 256 * 7 outputs. It writes the tile's differentials plus an
// 88-value halo to LDS once (two global reads per differential, the second a cache hit), then every thread computes 7
// CONSECUTIVE outputs from a window of 7 + 88 LDS reads held in registers: 13.6 LDS reads per output instead of 57. The
// thread stride of 7 complex values is odd. The terms of every output are added in ascending header position, so a value does
// not depend on where its index falls in a tile or a call. MEASURED (notes/plsync.md): the compiler keeps the window loop as
// a run-time loop and turns the constexpr tap signs into a branch tree (1119 branches in the kernel), which makes it 21 times
// slower than a copy of the same bytes; notes/plsync_patches/metric_window_compile_time.patch restates the window as
// compile-time recursion (straight-line packed adds) and awaits its run on the device.
#include "plsync_hip.h"
#include "plsc_decode.hpp"
#include <cmath>
#include <cstring>

namespace dvbs2 {

namespace {

constexpr int kHist = kPlsyncHistory;
constexpr int kR = 7, kThreads = 256, kTile = kR * kThreads, kWin = kR + 88;
constexpr PlsyncTapBits kTaps = plsync_tap_bits();
enum { SEARCHING = 0, FOUND = 1, LOCKED = 2 }; // frame_sync_state_t, lib/pl_frame_sync.h

constexpr bool tap_minus(int k) { return k < 64 ? ((kTaps.lo >> k) & 1) != 0 : ((kTaps.hi >> (k - 64)) & 1) != 0; }

// symbol g of the stream whose index 0 is x[0]: the 89 symbols before it come from the handle's history
__device__ inline float2 stream_sym(const float2* __restrict__ x, const float2* __restrict__ hist, int n_syms, int g)
{
    if (g >= n_syms || g < -kHist) return make_float2(0.0f, 0.0f);
    return g >= 0 ? x[g] : hist[kHist + g];
}

__global__ __launch_bounds__(kThreads) void plsync_metric_kernel(const float2* __restrict__ x, int n_syms, const float2* __restrict__ hist2,
                                                                 const PlSyncState* __restrict__ st, float* __restrict__ metric)
{
    __shared__ float2 d[kTile + 88];
    const float2* __restrict__ hist = hist2 + st->hist_sel * kHist;
    const int t = threadIdx.x, tile0 = blockIdx.x * kTile;
    for (int i = t; i < kTile + 88; i += kThreads) {
        const int g = tile0 - 88 + i;
        const float2 a = stream_sym(x, hist, n_syms, g), p = stream_sym(x, hist, n_syms, g - 1);
        d[i] = make_float2(a.x * p.x + a.y * p.y, a.x * p.y - a.y * p.x); // conj(x[g]) x[g-1] (lib/pl_frame_sync.cc:99)
    }
    __syncthreads();
    float sr[kR], si[kR], pr[kR], pi[kR];
#pragma unroll
    for (int r = 0; r < kR; r++) sr[r] = si[r] = pr[r] = pi[r] = 0.0f;
#pragma unroll
    for (int j = 0; j < kWin; j++) {
        const float2 v = d[t * kR + j];
#pragma unroll
        for (int r = 0; r < kR; r++) {
            const int k = j - r + 1; // header position of this differential for output r
            if (k >= 1 && k <= 25) { // v * (+-j): (-+ im, +- re)
                if (tap_minus(k)) { sr[r] += v.y; si[r] -= v.x; } else { sr[r] -= v.y; si[r] += v.x; }
            } else if (k >= 27 && k <= 89 && (k & 1)) {
                if (tap_minus(k)) { pr[r] += v.y; pi[r] -= v.x; } else { pr[r] -= v.y; pi[r] += v.x; }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kR; r++) {
        const int n = tile0 + t * kR + r;
        if (n < n_syms) {
            const float ar = sr[r] + pr[r], ai = si[r] + pi[r], br = sr[r] - pr[r], bi = si[r] - pi[r];
            const float a2 = ar * ar + ai * ai, b2 = br * br + bi * bi;
            metric[n] = sqrtf(a2 > b2 ? a2 : b2); // max(|S + P|, |S - P|) (:148-150)
        }
    }
}

// one wavefront; at most n_syms + 2 passes of the loop, each of which moves forward or ends it
__global__ __launch_bounds__(64) void plsync_track_kernel(const float2* __restrict__ x, int n_syms, const float* __restrict__ metric,
                                                          float2* __restrict__ hist2, PlSyncState* __restrict__ st,
                                                          const uint8_t* __restrict__ rank, PlSyncFrame* __restrict__ frames, int max_frames,
                                                          int fixed_plsc, int unlock_thresh, int coherent, int soft)
{
    const int l = threadIdx.x;
    const PlSyncState s = *st;
    const float2* __restrict__ hist = hist2 + s.hist_sel * kHist;
    const int64_t base = s.abs_base;
    int state = s.state, frame_len = s.frame_len, unlock = s.unlock_cnt, nf = 0, consumed = n_syms, hold = s.hold;
    int64_t last_peak = s.abs_last_peak, next = s.abs_next;

    for (int pass = 0; pass < n_syms + 2; pass++) {
        int n;
        if (state == LOCKED) {
            // once locked, only the index where the next peak is expected is looked at (:89-92, :127-128)
            const int64_t rel = last_peak + frame_len - base;
            if (rel >= n_syms) { if (hold) consumed = 0; break; } // a pending frame stays pending: its SOF is not consumed
            if (rel < 0) { state = SEARCHING; unlock = 0; continue; } // the caller skipped symbols: nothing to infer from
            n = (int)rel;
        } else {
            const int64_t rel = next - base;
            const int pos = rel < 0 ? 0 : rel > n_syms ? n_syms : (int)rel;
            if (pos >= n_syms) {
                if (hold) consumed = 0; // the buffer ends before the pending header's index: keep the SOF, resume where we were
                else next = base + n_syms;
                break;
            }
            const float m = pos + l < n_syms ? metric[pos + l] : 0.0f;
            const unsigned long long hit = __ballot(m > kPlsyncThresholdUnlocked);
            if (!hit) { next = base + (pos + 64 < n_syms ? pos + 64 : n_syms); continue; }
            n = pos + __ffsll((long long)hit) - 1;
        }
        const float m = metric[n];
        const bool is_peak = state == LOCKED ? m > kPlsyncThresholdLocked : m > kPlsyncThresholdUnlocked; // :168-169
        int ns = state, nu = unlock;
        if (is_peak) { // :183-193
            if (state == SEARCHING) ns = FOUND;
            else if (state == FOUND && base + n - last_peak == (int64_t)frame_len) ns = LOCKED;
            nu = 0;
        } else { // a peak was expected (:201-217)
            nu = unlock + 1;
            if (nu == unlock_thresh) { ns = SEARCHING; nu = 0; }
        }
        if (ns != SEARCHING) { // :242: this is the last symbol of a PLHEADER, real or inferred; handle it (plsync_cc_impl.cc:880)
            int plsc = fixed_plsc;
            if (plsc < 0) {
                const float2 h0 = stream_sym(x, hist, n_syms, n - 89 + l);
                const float2 sof = plsc::sof_sum(h0, l);
                const float2 xa = stream_sym(x, hist, n_syms, n - 63 + l), xb = stream_sym(x, hist, n_syms, n - 64 + l);
                plsc = plsc::decode_wave(xa, xb, atan2f(sof.y, sof.x), l, rank, coherent, soft);
            }
            const int new_len = pl_frame_shape(plsc).plframe_len, sof_idx = n - 89;
            if (nf >= max_frames || (int64_t)sof_idx + new_len + 90 > n_syms) {
                // not reportable yet: leave the machine as it was before this index and ask for the stream from this SOF
                consumed = sof_idx < 0 ? 0 : sof_idx;
                next = base + n;
                hold = 1;
                break;
            }
            if (l == 0) {
                PlSyncFrame f;
                f.sof_index = base + sof_idx; f.metric = m; f.plsc = (uint8_t)plsc;
                f.flags = (uint8_t)((is_peak ? 1 : 0) | (ns == LOCKED ? 2 : 0)); f.reserved[0] = f.reserved[1] = 0;
                frames[nf] = f;
            }
            nf++;
            frame_len = new_len; // set_frame_len (plsync_cc_impl.cc:594)
        }
        state = ns; unlock = nu; last_peak = base + n; next = base + n + 1; // :229: the count restarts
        hold = 0;
    }

    // the 89 symbols before the consumed point, into the history the state does not select
    float2* __restrict__ nh = hist2 + (1 - s.hist_sel) * kHist;
    for (int i = l; i < kHist; i += 64) nh[i] = stream_sym(x, hist, n_syms, consumed - kHist + i);
    if (l == 0) {
        PlSyncState o = s;
        o.last_base = base; o.abs_base = base + consumed; o.abs_last_peak = last_peak; o.abs_next = next;
        o.state = state; o.frame_len = frame_len; o.unlock_cnt = unlock; o.hist_sel = 1 - s.hist_sel;
        o.last_n_syms = n_syms; o.last_n_frames = nf; o.last_consumed = consumed; o.hold = hold;
        *st = o;
    }
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
    auto selected = [&](int i) { // locked, of the wanted PLSC, and whole (with the header after it) inside the searched buffer
        if (i >= nrec) return false;
        const PlSyncFrame r = frames[i];
        const int64_t rel = r.sof_index - base;
        return (r.flags & 2) && r.plsc == wanted && rel >= 0 && rel + len + 90 <= (int64_t)n_syms;
    };
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
    const float2* __restrict__ src = x + (frames[f].sof_index - base);
    float2* __restrict__ dst = out + (size_t)before * len;
    if (((uintptr_t)dst & 15) == 0) { // 16-byte stores; 16-byte loads too where the source allows (n is even)
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
        if (((uintptr_t)src & 15) == 0) {
            const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
            for (int i = t; i < n / 2; i += 256) d4[i] = s4[i];
        } else {
            for (int i = t; i < n / 2; i += 256) { const float2 a = src[2 * i], b = src[2 * i + 1]; d4[i] = make_float4(a.x, a.y, b.x, b.y); }
        }
    } else {
        for (int i = t; i < n; i += 256) dst[i] = src[i];
    }
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
                       d_state_, d_rank_, d_frames, max_frames_, fixed_plsc_, unlock_thresh_, coherent_, soft_);
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
