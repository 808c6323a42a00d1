// plsync_device.hpp -- the device code of the PLFRAME search, shared by the single-stream kernels (plsync_hip.hip) and the batched
// ones (plsync_batch_hip.hip): a metric tile, the tracker of one stream in one wavefront, the selection rule and the copy of the
// gather step. A kernel of either file only works out which stream and which tile it has and calls these, so a stream's results
// are the same bits through both. See plsync_hip.h for what they compute.
//
// Metric: a workgroup of 256 threads owns a tile of 256 * 7 outputs. It writes the tile's differentials plus an 88-value halo to
// LDS once (two global reads per differential, the second a cache hit), then every thread computes 7 CONSECUTIVE outputs from a
// window of 7 + 88 LDS reads held in registers: 13.6 LDS reads per output instead of 57. The thread stride of 7 complex values is
// odd. The terms of every output are added in ascending header position, so a value does not depend on where its index falls in
// a tile or a call. MEASURED (notes/plsync.md): the compiler keeps the window loop as a run-time loop and turns the constexpr tap
// signs into a branch tree (1119 branches in the kernel), which makes it 21 times slower than a copy of the same bytes;
// notes/plsync_patches/metric_window_compile_time.patch restates the window as compile-time recursion (straight-line packed adds)
// and awaits its run on the device.
#pragma once
#include "plsync_hip.h"
#include "plsc_decode.hpp"

namespace dvbs2 {
namespace plsync_dev {

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

// the tile of outputs that starts at index tile0 (a multiple of kTile), by a whole workgroup of kThreads; hist: the selected history
__device__ inline void metric_tile(const float2* __restrict__ x, int n_syms, const float2* __restrict__ hist, int tile0, float* __restrict__ metric)
{
    __shared__ float2 d[kTile + 88];
    const int t = threadIdx.x;
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

struct TrackArgs { int max_frames, fixed_plsc, unlock_thresh, coherent, soft; };
struct TrackResult { int n_frames, consumed, state; }; // what the state's last_n_frames, last_consumed and state became, in every lane

// one stream in one wavefront: x, metric, hist2 (2 x 89), st and frames are that stream's; at most n_syms + 2 passes of the loop,
// each of which moves forward or ends it
__device__ inline TrackResult track_wave(const float2* __restrict__ x, int n_syms, const float* __restrict__ metric, float2* __restrict__ hist2,
                                  PlSyncState* __restrict__ st, const uint8_t* __restrict__ rank, PlSyncFrame* __restrict__ frames, const TrackArgs a)
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
            if (nu == a.unlock_thresh) { ns = SEARCHING; nu = 0; }
        }
        if (ns != SEARCHING) { // :242: this is the last symbol of a PLHEADER, real or inferred; handle it (plsync_cc_impl.cc:880)
            int plsc = a.fixed_plsc;
            if (plsc < 0) {
                const float2 h0 = stream_sym(x, hist, n_syms, n - 89 + l);
                const float2 sof = plsc::sof_sum(h0, l);
                const float2 xa = stream_sym(x, hist, n_syms, n - 63 + l), xb = stream_sym(x, hist, n_syms, n - 64 + l);
                plsc = plsc::decode_wave(xa, xb, atan2f(sof.y, sof.x), l, rank, a.coherent, a.soft);
            }
            const int new_len = pl_frame_shape(plsc).plframe_len, sof_idx = n - 89;
            if (nf >= a.max_frames || (int64_t)sof_idx + new_len + 90 > n_syms) {
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
    return TrackResult{ nf, consumed, state };
}

// what gather takes: locked, of the wanted PLSC, and whole (with the header after it) inside the searched buffer
__device__ inline bool gather_selects(const PlSyncFrame r, int64_t base, int n_syms, int wanted, int len)
{
    const int64_t rel = r.sof_index - base;
    return (r.flags & 2) && r.plsc == wanted && rel >= 0 && rel + len + 90 <= (int64_t)n_syms;
}

// n symbols (even) by a workgroup of 256: 16-byte stores where dst allows, 16-byte loads too where the source allows
__device__ inline void gather_copy(const float2* __restrict__ src, float2* __restrict__ dst, int n, int t)
{
    if (((uintptr_t)dst & 15) == 0) {
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
}

} // namespace plsync_dev
} // namespace dvbs2
