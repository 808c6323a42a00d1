// resamp_hip.hip -- see resamp_hip.h.
#include "resamp_hip.h"
#include "stream_device.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off) // the arithmetic is pinned: a product, then an addition (the library is built -ffp-contract=off as well)

namespace dvbs2 {

int resamp_step(double rate, uint64_t* step)
{
    if (!step || !(rate >= 0.5 && rate <= 64.0)) return -1;
    *step = (uint64_t)std::nearbyint(4294967296.0 / rate);
    return 0;
}

int resamp_geometry(int nfilts, int ntaps, int* L, int* history, int* delay_num)
{
    if (nfilts < 2 || nfilts > 256 || (nfilts & (nfilts - 1)) || ntaps < 1 || ntaps > kResampMaxTaps) return -1;
    const int terms = (ntaps + nfilts - 1) / nfilts;
    if (terms > kResampMaxTerms) return -1;
    if (L) *L = terms;
    if (history) *history = terms - 1;
    if (delay_num) *delay_num = (ntaps - 1) / 2;
    return 0;
}

int64_t resamp_max_out(uint64_t step, int n_in)
{
    if (step < kResampMinStep || step > kResampMaxStep || n_in < 0 || n_in > kResampMaxSamples) return -1;
    return resamp_advance(0, step, n_in, nullptr);
}

namespace {

constexpr int kSpan = 2 * kResampTile + kResampMaxTerms; // LDS slots for samples: at step <= 2^33 a tile's outputs span at most
                                                         // 2 (kResampTile - 1) + 1 newest samples, and L - 1 <= 127 before the first
constexpr int kStage = (kSpan + 255) / 256;              // slots a thread fills
// pairs in the largest bank: nfilts rows of L | 1 <= L + 1 pairs, nfilts L <= ntaps + nfilts - 1, an even count
constexpr int kMaxBank = kResampMaxTaps + 2 * 256;

struct ResampGeom {
    int32_t nfilts, lg, ntaps, L, row; // row: pairs per branch in the bank
    int32_t bank_quads;                // the bank in 16-byte units (two pairs)
};

// Block (blockIdx.x, blockIdx.y) writes outputs [blockIdx.x * kResampTile, + kResampTile) of stream blockIdx.y, those of them that lie in
// the call (T < N). LDS: slot q holds x[i0 - (L - 1) + q], i0 the newest sample of the tile's first output; behind kSpan slots the bank.
// Nothing is read at or past n_in or before the history, nothing written at or past the stream's n_out.
__global__ __launch_bounds__(256) void resamp_kernel(const float2* __restrict__ in, long long in_stride, const float2* __restrict__ hist,
                                                     const float4* __restrict__ bank, const unsigned long long* __restrict__ acc,
                                                     unsigned long long step, int n_in, float2* __restrict__ out, long long out_stride,
                                                     ResampGeom g)
{
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int t = threadIdx.x, H = g.L - 1;
    const unsigned long long N = (unsigned long long)n_in << 32;
    const unsigned long long base = (unsigned long long)blockIdx.x * kResampTile;
    const unsigned long long T0 = acc[blockIdx.y] + base * step; // the tile's first output
    if (T0 >= N) return;                                          // (the whole block: the stream has fewer outputs than the longest)
    const int i0 = (int)(T0 >> 32);                               // < n_in
    const unsigned int f0 = (unsigned int)T0;
    // the newest sample of the tile's last output, counted from i0, clipped to the call: at most 2 (kResampTile - 1)
    const int last = min((int)((f0 + (unsigned long long)(kResampTile - 1) * step) >> 32), n_in - 1 - i0);
    const int n_slots = last + 1 + H; // <= kSpan - 1
    const float2* __restrict__ x = in + (long long)blockIdx.y * in_stride;
    const float2* __restrict__ h0 = hist + (long long)blockIdx.y * H;
    float2 stage[kStage]; // every load of the thread in flight before the first LDS write
#pragma unroll
    for (int c = 0; c < kStage; c++) {
        const int q = t + 256 * c, i = i0 - H + q; // the LDS slot and the sample's index in the call; i + H = i0 + q >= 0
        if (q < n_slots) stage[c] = history_or_input(h0, x, H, i);
    }
    float4* __restrict__ lb4 = reinterpret_cast<float4*>(lds + kSpan);
    for (int e = t; e < g.bank_quads; e += 256) lb4[e] = bank[e];
#pragma unroll
    for (int c = 0; c < kStage; c++)
        if (t + 256 * c < n_slots) lds[t + 256 * c] = stage[c];
    __syncthreads();

    const float2* __restrict__ lb = lds + kSpan;
    float2* __restrict__ y = out + (long long)blockIdx.y * out_stride + (long long)base;
    const unsigned long long whole = T0 - f0;
    for (int m = t; m < kResampTile; m += 256) {
        const unsigned long long tt = f0 + (unsigned long long)m * step; // T - (i0 << 32): below 2^43
        if (whole + tt >= N) break;                                       // T grows with m
        const int r = (int)(tt >> 32);                                    // <= last
        const unsigned int f = (unsigned int)tt;
        const int j = (int)(f >> (32 - g.lg));
        const float a = (float)((f << g.lg) >> 8) * 0x1p-24f;
        const float2* __restrict__ xs = lds + H + r; // xs[-k] = x[i - k]; k <= H
        const float2* __restrict__ b = lb + j * g.row;
        v2f o0 = { 0.0f, 0.0f }, o1 = { 0.0f, 0.0f };
        for (int k = 0; k < H; k++) { // every branch has these L - 1 terms
            const float2 xv = xs[-k], hd = b[k];
            const v2f v = { xv.x, xv.y };
            o0 = o0 + v * hd.x;
            o1 = o1 + v * hd.y;
        }
        if (j + H * g.nfilts < g.ntaps) { // and the branches below ntaps - (L - 1) nfilts one more
            const float2 xv = xs[-H], hd = b[H];
            const v2f v = { xv.x, xv.y };
            o0 = o0 + v * hd.x;
            o1 = o1 + v * hd.y;
        }
        const v2f o = o0 + o1 * a;
        y[m] = make_float2(o.x, o.y);
    }
}

// One block per stream behind resamp_kernel on the same HIP stream: roll_history over the call's samples (H <= 127), and the stream's
// position after the call.
__global__ __launch_bounds__(128) void resamp_state_kernel(const float2* __restrict__ in, long long in_stride, float2* __restrict__ hist,
                                                           unsigned long long* __restrict__ acc, unsigned long long step, int n_in, int H)
{
    const float2* __restrict__ x = in + (long long)blockIdx.x * in_stride;
    roll_history<128, 1>(hist + (long long)blockIdx.x * H, H, n_in, [&](long long j) { return x[j]; });
    if (threadIdx.x == 0) {
        const unsigned long long N = (unsigned long long)n_in << 32, a = acc[blockIdx.x];
        const unsigned long long n = a >= N ? 0 : (N - a + step - 1) / step;
        acc[blockIdx.x] = a + n * step - N;
    }
}

} // namespace

std::string ResamplerHip::check_args(int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples)
{
    if (nfilts < 2 || nfilts > 256 || (nfilts & (nfilts - 1))) return "nfilts must be a power of two in 2..256";
    if (ntaps < 1 || ntaps > kResampMaxTaps || (ntaps + nfilts - 1) / nfilts > kResampMaxTerms)
        return "ntaps must be in 1..8192 with at most 128 taps per branch (ceil(ntaps / nfilts) <= 128)";
    if (const std::string bad = check_taps(taps, ntaps, "taps"); !bad.empty()) return bad;
    uint64_t step;
    if (resamp_step(rate, &step)) return "rate must lie in [0.5, 64]";
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535: streams are one launch dimension)";
    if (max_samples < 1 || max_samples > kResampMaxSamples) return "max_samples out of range (1..2^24)";
    return "";
}

ResamplerHip::ResamplerHip(int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = check_args(nfilts, taps, ntaps, rate, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    nfilts_ = nfilts; ntaps_ = ntaps; L_ = (ntaps + nfilts - 1) / nfilts;
    while ((1 << lg_) < nfilts) lg_++;
    resamp_step(rate, &step_);
    // An odd row: branch j starts at pair j row, so the branches a half-wave reads in one instruction fall on different 8-byte slots of the
    // 32 that an LDS row has as long as they differ modulo 32. An even count of pairs in all, for 16-byte copies.
    row_ = L_ | 1;
    bank_elems_ = (nfilts_ * row_ + 1) & ~1;
    std::vector<float2> bank((size_t)bank_elems_, make_float2(0.0f, 0.0f));
    for (int n = 0; n < ntaps; n++) {
        const float d = n + 1 < ntaps ? taps[n + 1] - taps[n] : 0.0f; // create_diff_taps: one float subtraction each
        bank[(size_t)(n % nfilts) * row_ + n / nfilts] = make_float2(taps[n], d);
    }
    acc_.assign((size_t)max_streams_, 0);
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the bank", alloc(&d_bank_, (size_t)bank_elems_));
    HIP_OK_AS("hipMalloc of the histories", alloc_zeroed(&d_hist_, (size_t)max_streams_ * std::max(L_ - 1, 1)));
    HIP_OK_AS("hipMalloc of the positions", alloc_zeroed(&d_acc_, (size_t)max_streams_));
    HIP_OK(hipMemcpy(d_bank_, bank.data(), bank.size() * sizeof(float2), hipMemcpyHostToDevice));
    // The largest bank is above the 64 KiB a kernel gets unasked. The attribute belongs to the kernel, not to the handle: always the cap
    HIP_OK(hipFuncSetAttribute((const void*)resamp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((kSpan + kMaxBank) * sizeof(float2))));
}

int ResamplerHip::set_step(uint64_t step)
{
    call_err_ = {};
    if (step < kResampMinStep || step > kResampMaxStep) { call_err_.argument("step must lie in [2^26, 2^33]"); return -1; }
    step_ = step;
    return 0;
}

int64_t ResamplerHip::produce(int n_in, int n_streams, int64_t* n_out) const
{
    int64_t most = 0;
    for (int s = 0; s < n_streams; s++) {
        const int64_t n = resamp_advance(acc_[s], step_, n_in, nullptr);
        if (n_out) n_out[s] = n;
        most = std::max(most, n);
    }
    return most;
}

int ResamplerHip::reset()
{
    if (reset_phase(nullptr)) return -1; // (waits for the device)
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(zero(d_hist_));
    return 0;
}

int ResamplerHip::reset_phase(const uint32_t* frac)
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    std::vector<uint64_t> acc((size_t)max_streams_, 0);
    for (int s = 0; frac && s < max_streams_; s++) acc[s] = frac[s];
    HIP_RET(hipMemcpy(d_acc_, acc.data(), acc.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    acc_ = acc;
    return 0;
}

int ResamplerHip::state(uint64_t* acc)
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(hipMemcpy(acc, d_acc_, (size_t)max_streams_ * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int ResamplerHip::process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_in == 0 || n_streams == 0) return 0; // no output, and acc' = acc
    const int64_t most = produce(n_in, n_streams, nullptr);
    const ResampGeom g = { nfilts_, lg_, ntaps_, L_, row_, bank_elems_ / 2 };
    const size_t lds = ((size_t)kSpan + bank_elems_) * sizeof(float2);
    if (most > 0) {
        const dim3 grid((unsigned)((most + kResampTile - 1) / kResampTile), n_streams);
        hipLaunchKernelGGL(resamp_kernel, grid, dim3(256), lds, stream, reinterpret_cast<const float2*>(d_in), (long long)in_stride, d_hist_,
                           reinterpret_cast<const float4*>(d_bank_), d_acc_, (unsigned long long)step_, n_in, reinterpret_cast<float2*>(d_out),
                           (long long)out_stride, g);
        if (launched("resamp kernel launch")) return -1;
    }
    hipLaunchKernelGGL(resamp_state_kernel, dim3(n_streams), dim3(128), 0, stream, reinterpret_cast<const float2*>(d_in), (long long)in_stride,
                       d_hist_, d_acc_, (unsigned long long)step_, n_in, L_ - 1);
    if (launched("resamp state kernel launch")) return -1;
    for (int s = 0; s < n_streams; s++) resamp_advance(acc_[s], step_, n_in, &acc_[s]);
    return 0;
}

} // namespace dvbs2
