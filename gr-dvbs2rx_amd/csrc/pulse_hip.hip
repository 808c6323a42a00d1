// pulse_hip.hip -- see pulse_hip.h.
#include "pulse_hip.h"
#include "rrc_pulse.h"
#include "stream_device.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off) // the arithmetic is pinned: a product, then an addition (the library is built -ffp-contract=off as well)

namespace dvbs2 {

int pulse_geometry(int sps, int rrc_delay, int* ntaps, int* history, int* delay)
{
    if (sps < 2 || (sps & 1) || sps > 64 || rrc_delay < 1 || rrc_delay > 64) return -1;
    const int n = 2 * sps * rrc_delay + 1;
    if (ntaps) *ntaps = n;
    if (history) *history = (n + sps - 1) / sps - 1;
    if (delay) *delay = sps * rrc_delay;
    return 0;
}

int pulse_taps(int sps, float rolloff, int rrc_delay, double tau, double gain, float* taps)
{
    int n;
    if (!taps || pulse_geometry(sps, rrc_delay, &n, nullptr, nullptr) || !(rolloff >= 0.0f && rolloff <= 1.0f) || !(std::fabs(tau) <= 0.5) ||
        !std::isfinite(gain) || gain == 0.0)
        return -1;
    const int centre = (n - 1) / 2;
    double sum = 0.0; // of the taps at tau = 0: a shift moves the pulse and leaves its scale alone
    for (int i = 0; i < n; i++) sum += rrc((double)(i - centre) / sps, (double)rolloff);
    for (int i = 0; i < n; i++) taps[i] = (float)(rrc((double)(i - centre) / sps - tau, (double)rolloff) * gain / sum);
    return 0;
}

int pulse_scale_taps(float* taps, int ntaps, int sps, double fullscale)
{
    if (!taps || ntaps < 1 || sps < 1 || !std::isfinite(fullscale)) return -1;
    double max_sum = 0.0;
    for (int p = 0; p < sps && p < ntaps; p++) {
        double sum = 0.0;
        for (int i = p; i < ntaps; i += sps) sum += std::fabs((double)taps[i]);
        if (!std::isfinite(sum)) return -1;
        max_sum = std::max(max_sum, sum);
    }
    if (max_sum == 0.0) return -1;
    for (int i = 0; i < ntaps; i++) taps[i] = (float)(std::sqrt(2.0) * fullscale * (double)taps[i] / max_sum);
    return 0;
}

namespace {

struct PulseGeom {
    int32_t sps, ntaps, history;
    int32_t full, rest; // ntaps = full * sps + rest, rest < sps: phase p has full + (p < rest) terms
    uint32_t inv_sps;   // ceil(2^32 / sps): n / sps = umulhi(n, inv_sps) for n < kPulseTile * 64
};

constexpr int kStage = (kPulseTile + kPulseMaxTerms - 1 + 255) / 256; // LDS slots a thread fills: tile and history over 256 threads

// Block (blockIdx.x, blockIdx.y) shapes symbols [blockIdx.x * kPulseTile, + kPulseTile) of stream blockIdx.y. LDS: the tile's symbols behind
// the `history` symbols before them (slot j holds x[base - history + j]), then, unless kUniform, the taps. Nothing is read past n_syms,
// nothing written past n_syms * sps. kUniform: sps == 2, every pair has phase 0; kWide: every pair's address is a multiple of 16 bytes.
template <bool kUniform, bool kWide>
__global__ __launch_bounds__(256) void pulse_kernel(const float2* __restrict__ in, long long in_stride, const float2* __restrict__ hist,
                                                    const float* __restrict__ taps, float2* __restrict__ out, long long out_stride,
                                                    int n_syms, PulseGeom g)
{
    extern __shared__ float2 lds[];
    const int t = threadIdx.x, H = g.history, sps = kUniform ? 2 : g.sps;
    const int base = blockIdx.x * kPulseTile;
    const int n_here = min(kPulseTile, n_syms - base);
    const float2* __restrict__ x = in + (long long)blockIdx.y * in_stride;
    const float2* __restrict__ h0 = hist + (long long)blockIdx.y * H;
    float2 stage[kStage]; // every load of the thread in flight before the first LDS write
#pragma unroll
    for (int c = 0; c < kStage; c++) {
        const int j = t + 256 * c, i = base - H + j; // the LDS slot and the symbol's index in the call
        if (j < n_here + H) stage[c] = history_or_input(h0, x, H, i);
    }
#pragma unroll
    for (int c = 0; c < kStage; c++)
        if (t + 256 * c < n_here + H) lds[t + 256 * c] = stage[c];
    float* lt = reinterpret_cast<float*>(lds + kPulseTile + H);
    if (!kUniform)
        for (int i = t; i < g.ntaps; i += 256) lt[i] = taps[i];
    __syncthreads();

    float2* __restrict__ y = out + (long long)blockIdx.y * out_stride + (long long)base * sps;
    const int n_pairs = n_here * (sps >> 1);
    for (int q = t; q < n_pairs; q += 256) {
        const int n = 2 * q;                                  // first sample of the pair, counted from the tile's start
        const int m = kUniform ? q : (int)__umulhi((uint32_t)n, g.inv_sps); // its symbol
        const int p = kUniform ? 0 : n - m * sps;             // its phase: even, p + 1 < sps
        const int n1 = g.full + (p + 1 < g.rest ? 1 : 0);     // terms of the second sample; the first has one more when p == rest - 1
        const bool more = p < g.rest && !(p + 1 < g.rest);
        const float2* __restrict__ xs = lds + H + m;           // xs[-k] = x[m - k]; k <= history
        v2f a0 = { 0.0f, 0.0f }, a1 = { 0.0f, 0.0f };
        for (int k = 0; k < n1; k++) {
            const float2 xv = xs[-k];
            const v2f v = { xv.x, xv.y };
            const float c0 = kUniform ? taps[2 * k] : lt[p + k * sps], c1 = kUniform ? taps[2 * k + 1] : lt[p + 1 + k * sps];
            a0 = a0 + v * c0;
            a1 = a1 + v * c1;
        }
        if (more) {
            const float2 xv = xs[-n1];
            const v2f v = { xv.x, xv.y };
            a0 = a0 + v * (kUniform ? taps[2 * n1] : lt[p + n1 * sps]);
        }
        if (kWide) *reinterpret_cast<float4*>(y + n) = make_float4(a0.x, a0.y, a1.x, a1.y);
        else { y[n] = make_float2(a0.x, a0.y); y[n + 1] = make_float2(a1.x, a1.y); }
    }
}

// One block per stream behind pulse_kernel on the same HIP stream: roll_history over the call's symbols. H <= 128.
__global__ __launch_bounds__(128) void pulse_history_kernel(const float2* __restrict__ in, long long in_stride, float2* __restrict__ hist,
                                                            int n_syms, int H)
{
    const float2* __restrict__ x = in + (long long)blockIdx.x * in_stride;
    roll_history<128, 1>(hist + (long long)blockIdx.x * H, H, n_syms, [&](long long j) { return x[j]; });
}

} // namespace

std::string PulseShaperHip::check_args(int sps, const float* taps, int ntaps, int max_streams, int max_symbols)
{
    if (sps < 2 || (sps & 1) || sps > 64) return "sps must be an even integer in 2..64";
    if (ntaps < 1 || (ntaps + sps - 1) / sps > kPulseMaxTerms) return "ntaps must be at least 1 and at most 129 taps per phase (ceil(ntaps / sps) <= 129)";
    if (const std::string bad = check_taps(taps, ntaps, "taps"); !bad.empty()) return bad;
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535: streams are one launch dimension)";
    if (max_symbols < 1 || max_symbols > (1 << 30)) return "max_symbols out of range (1..2^30)";
    return "";
}

PulseShaperHip::PulseShaperHip(int sps, const float* taps, int ntaps, int max_streams, int max_symbols, int device)
    : StreamStage(max_streams, max_symbols, device)
{
    if (const std::string bad = check_args(sps, taps, ntaps, max_streams, max_symbols); !bad.empty()) { err_.argument(bad); return; }
    sps_ = sps; ntaps_ = ntaps; history_ = (ntaps + sps - 1) / sps - 1;
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the taps", alloc(&d_taps_, (size_t)ntaps));
    HIP_OK_AS("hipMalloc of the histories", alloc_zeroed(&d_hist_, (size_t)max_streams_ * std::max(history_, 1)));
    HIP_OK(hipMemcpy(d_taps_, taps, (size_t)ntaps * sizeof(float), hipMemcpyHostToDevice));
}

int PulseShaperHip::reset()
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(zero(d_hist_));
    return 0;
}

int PulseShaperHip::shape_device(const float* d_in, int64_t in_stride, int n_syms, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_syms == 0 || n_streams == 0) return 0;
    const PulseGeom g = { sps_, ntaps_, history_, ntaps_ / sps_, ntaps_ % sps_, (uint32_t)(((1ull << 32) + sps_ - 1) / sps_) };
    // a pair starts at an even sample: 16-byte aligned when the base is and every stream starts at an even element
    const bool wide = ((uintptr_t)d_out & 15) == 0 && (n_streams == 1 || (out_stride & 1) == 0);
    const bool uniform = sps_ == 2;
    const size_t lds = (size_t)(kPulseTile + history_) * sizeof(float2) + (uniform ? 0 : (size_t)ntaps_ * sizeof(float));
    const dim3 grid((n_syms + kPulseTile - 1) / kPulseTile, n_streams);
    auto kernel = uniform ? (wide ? pulse_kernel<true, true> : pulse_kernel<true, false>) : (wide ? pulse_kernel<false, true> : pulse_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, reinterpret_cast<const float2*>(d_in), (long long)in_stride, d_hist_, d_taps_,
                       reinterpret_cast<float2*>(d_out), (long long)out_stride, n_syms, g);
    if (launched("pulse kernel launch")) return -1;
    if (history_ > 0) {
        hipLaunchKernelGGL(pulse_history_kernel, dim3(n_streams), dim3(128), 0, stream, reinterpret_cast<const float2*>(d_in), (long long)in_stride,
                           d_hist_, n_syms, history_);
        if (launched("pulse history kernel launch")) return -1;
    }
    return 0;
}

} // namespace dvbs2
