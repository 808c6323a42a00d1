// ddc_hip.hip -- see ddc_hip.h.
#include "ddc_hip.h"
#include "rotator_turns.h"
#include "rotator_math.hpp"
#include "stream_device.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off) // the arithmetic is pinned: a product, then an addition (the library is built -ffp-contract=off as well)

namespace dvbs2 {

int ddc_geometry(int decim, int ntaps, int* history, int* delay_num)
{
    if (decim < 1 || decim > kDdcMaxDecim || ntaps < 1 || ntaps > kDdcMaxTaps) return -1;
    if (history) *history = ntaps - 1;
    if (delay_num) *delay_num = ntaps - 1;
    return 0;
}

int64_t ddc_produce(int64_t position, int decim, int n_in)
{
    if (position < 0 || position > kDdcMaxPosition || decim < 1 || decim > kDdcMaxDecim || n_in < 0 || n_in > kDdcMaxSamples) return -1;
    const int64_t end = position + n_in;
    return (end + decim - 1) / decim - (position + decim - 1) / decim;
}

namespace {

constexpr int kMaxLds = kDdcSpan + 2 * kDdcMaxDecim; // LDS slots at most: the span rounded up to whole columns, and one more column
constexpr int kHistPerThread = (kDdcMaxTaps - 1 + 255) / 256;

struct DdcGeom {
    int32_t D, ntaps, tile;
    int32_t cols;     // LDS columns: ceil(span / D) made odd, so that the rows a half-wave writes in one instruction fall on different banks
    int32_t hq, hr;   // ntaps - 1 = hq D + hr: row and column of the newest sample of the tile's first output
    uint32_t inv_D;   // ceil(2^32 / D) for D > 1: s / D = umulhi(s, inv_D) for s < 2^16
};

// Block (blockIdx.x, blockIdx.y) writes outputs [blockIdx.y * tile, + tile) of the call for channel blockIdx.x, those of them below
// n_out. Output o of the call uses the call's input samples r0 + o D - t, t < ntaps. LDS: slot s holds the mixed sample of index
// i0 + s relative to the call, i0 = r0 + o0 D - (ntaps - 1) >= -(ntaps - 1), at row s mod D and column s div D. Nothing is read at or
// past n_in (the last output's newest sample is below it) or before the history, nothing written at or past n_out.
template <int R>
__global__ __launch_bounds__(256) void ddc_kernel(const float2* __restrict__ in, long long in_stride, const float2* __restrict__ hist,
                                                  const float* __restrict__ taps, const DdcHip::Chan* __restrict__ table,
                                                  const unsigned long long* __restrict__ phase, int r0, int n_out,
                                                  float2* __restrict__ out, long long out_stride, DdcGeom g)
{
    extern __shared__ float2 lds[];
    const int t = threadIdx.x, c = blockIdx.x, D = g.D, H = g.ntaps - 1;
    const int o0 = blockIdx.y * g.tile;
    const int n_here = min(g.tile, n_out - o0);  // >= 1: the grid has ceil(n_out / tile) rows
    const int n_slots = H + (n_here - 1) * D + 1; // <= kDdcSpan
    const int i0 = r0 + o0 * D - H;
    const DdcHip::Chan ch = table[c];
    const uint64_t P = phase[c];
    const float2* __restrict__ x = in + (long long)ch.input * in_stride;
    const float2* __restrict__ h0 = hist + (long long)c * H;
#pragma unroll 4
    for (int s = t; s < n_slots; s += 256) {
        const int i = i0 + s; // -H <= i < n_in
        const float2 z = i < 0 ? h0[i + H] : rotate_one(x[i], P + (uint64_t)(uint32_t)i * ch.inc);
        const int col = D == 1 ? s : (int)__umulhi((uint32_t)s, g.inv_D), row = s - col * D;
        lds[row * g.cols + col] = z;
    }
    __syncthreads();

    float2* __restrict__ y = out + (long long)c * out_stride + o0;
    for (int j0 = 0; j0 < n_here; j0 += 256 * R) {
        int jj[R]; // the lane's outputs, counted from the tile's start; one past the tile's end repeats the last and is not stored
        v2f acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            jj[r] = min(j0 + t + 256 * r, n_here - 1);
            acc[r] = v2f{ 0.0f, 0.0f };
        }
        // tap 0 meets slot j D + (ntaps - 1), the last tap slot j D: one row up per tap, from row 0 to row D - 1 of the column before
        int row = g.hr, at = g.hr * g.cols + g.hq;
        const int up = -g.cols, wrap = (D - 1) * g.cols - 1;
#ifdef DVBS2_DDC_ONE_TAP // a measurement build (tools/ddc_time.py, notes/ddc.md): the FIR cut to its first tap, staging and mixing as they are
        const int n_fir = 1;
#else
        const int n_fir = g.ntaps;
#endif
        for (int tp = 0; tp < n_fir; tp++) {
            const float h = taps[tp];
            const float2* __restrict__ p = lds + at;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float2 zv = p[jj[r]];
                const v2f v = { zv.x, zv.y };
                acc[r] = acc[r] + v * h;
            }
            at += row == 0 ? wrap : up;
            row = row == 0 ? D - 1 : row - 1;
        }
#pragma unroll
        for (int r = 0; r < R; r++)
            if (j0 + t + 256 * r < n_here) y[j0 + t + 256 * r] = make_float2(acc[r].x, acc[r].y);
    }
}

// One block per channel behind ddc_kernel on the same HIP stream: roll_history over the call's samples, mixed once more with the same
// arithmetic (the history holds mixed samples; H <= 4095), and the channel's phase after the call.
__global__ __launch_bounds__(256) void ddc_state_kernel(const float2* __restrict__ in, long long in_stride, float2* __restrict__ hist,
                                                        const DdcHip::Chan* __restrict__ table, unsigned long long* __restrict__ phase,
                                                        int n_in, int H)
{
    const int c = blockIdx.x;
    const DdcHip::Chan ch = table[c];
    const uint64_t P = phase[c];
    const float2* __restrict__ x = in + (long long)ch.input * in_stride;
    roll_history<256, kHistPerThread>(hist + (long long)c * H, H, n_in, [&](long long j) { return rotate_one(x[j], P + (uint64_t)j * ch.inc); });
    if (threadIdx.x == 0) phase[c] = P + (uint64_t)n_in * ch.inc;
}

} // namespace

std::string DdcHip::check_args(int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples)
{
    if (decim < 1 || decim > kDdcMaxDecim) return "decim must be in 1..256";
    if (ntaps < 1 || ntaps > kDdcMaxTaps) return "ntaps must be in 1..4096";
    if (const std::string bad = check_taps(taps, ntaps, "taps"); !bad.empty()) return bad;
    if (max_channels < 1 || max_channels > 65535) return "max_channels out of range (1..65535)";
    if (max_inputs < 1 || max_inputs > 65535) return "max_inputs out of range (1..65535)";
    if (max_samples < 1 || max_samples > kDdcMaxSamples) return "max_samples out of range (1..2^24)";
    return "";
}

DdcHip::DdcHip(int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples, int device)
    : StreamStage(max_channels, max_samples, device), max_inputs_(max_inputs)
{
    if (const std::string bad = check_args(decim, taps, ntaps, max_channels, max_inputs, max_samples); !bad.empty()) { err_.argument(bad); return; }
    decim_ = decim; ntaps_ = ntaps; tile_ = ddc_tile(decim, ntaps);
    mirror_.phase.assign((size_t)max_channels, 0);
    mirror_.inc.assign((size_t)max_channels, 0);
    table_.assign((size_t)max_channels, Chan{ 0, 0, 0 });
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the taps", alloc(&d_taps_, (size_t)ntaps_));
    HIP_OK_AS("hipMalloc of the histories", alloc_zeroed(&d_hist_, (size_t)max_channels * std::max(ntaps_ - 1, 1)));
    HIP_OK_AS("hipMalloc of the phases", alloc_zeroed(&d_phase_, (size_t)max_channels));
    HIP_OK_AS("hipMalloc of the channel table", alloc(&d_table_, (size_t)max_channels));
    HIP_OK(hipMemcpy(d_taps_, taps, (size_t)ntaps_ * sizeof(float), hipMemcpyHostToDevice));
    // The largest span is above the 64 KiB a kernel gets unasked. The attribute belongs to the kernel, not to the handle: always the cap
    HIP_OK(hipFuncSetAttribute((const void*)ddc_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxLds * sizeof(float2))));
    HIP_OK(hipFuncSetAttribute((const void*)ddc_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxLds * sizeof(float2))));
    HIP_OK(hipFuncSetAttribute((const void*)ddc_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxLds * sizeof(float2))));
}

int DdcHip::set_channel(int channel, int input, double phase_inc)
{
    call_err_ = {};
    if (channel < 0 || channel >= max_channels()) { call_err_.argument("channel out of range"); return -1; }
    if (input < 0 || input >= max_inputs_) { call_err_.argument("input out of range"); return -1; }
    if (!std::isfinite(phase_inc)) { call_err_.argument("phase_inc must be finite"); return -1; }
    table_[channel] = Chan{ rotator_inc_turns(phase_inc), input, 0 };
    mirror_.inc[channel] = table_[channel].inc;
    table_dirty_ = true;
    return 0;
}

int DdcHip::reset()
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(zero(d_hist_));
    HIP_RET(zero(d_phase_));
    mirror_.counter = 0;
    std::fill(mirror_.phase.begin(), mirror_.phase.end(), 0);
    return 0;
}

int DdcHip::state(uint64_t* phases)
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(hipMemcpy(phases, d_phase_, (size_t)max_channels() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int DdcHip::process_device(const float* d_in, int64_t in_stride, int n_in, int n_channels, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_in == 0) return 0; // no output, and nothing moves
    const int64_t n_out = produce(n_in);
    if (n_out < 0) { call_err_.argument("the sample counter is exhausted"); return -1; }
    if (n_channels > 0) {
        if (table_dirty_) { // (pageable memory: the runtime has taken its copy when the call returns)
            HIP_RET(hipMemcpyAsync(d_table_, table_.data(), table_.size() * sizeof(Chan), hipMemcpyHostToDevice, stream));
            table_dirty_ = false;
        }
        const int D = decim_, H = ntaps_ - 1;
        if (n_out > 0) {
            const int r0 = (int)((D - mirror_.counter % D) % D); // the call's first output sits on its input sample r0
            const int span = H + (tile_ - 1) * D + 1;
            DdcGeom g = { D, ntaps_, tile_, ((span + D - 1) / D) | 1, H / D, H % D, D > 1 ? (uint32_t)(((1ull << 32) + D - 1) / D) : 0u };
            const size_t lds = (size_t)D * g.cols * sizeof(float2); // <= kMaxLds slots
            const dim3 grid(n_channels, (unsigned)((n_out + tile_ - 1) / tile_));
            auto kernel = tile_ > 512 ? ddc_kernel<4> : tile_ > 256 ? ddc_kernel<2> : ddc_kernel<1>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, reinterpret_cast<const float2*>(d_in), (long long)in_stride, d_hist_, d_taps_,
                               d_table_, d_phase_, r0, (int)n_out, reinterpret_cast<float2*>(d_out), (long long)out_stride, g);
            if (launched("ddc kernel launch")) return -1;
        }
        hipLaunchKernelGGL(ddc_state_kernel, dim3(n_channels), dim3(256), 0, stream, reinterpret_cast<const float2*>(d_in), (long long)in_stride,
                           d_hist_, d_table_, d_phase_, n_in, H);
        if (launched("ddc state kernel launch")) return -1;
    }
    mirror_.advance(n_in, n_channels);
    return 0;
}

} // namespace dvbs2
