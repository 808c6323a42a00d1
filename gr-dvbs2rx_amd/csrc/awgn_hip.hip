// awgn_hip.hip -- see awgn_hip.h.
#include "awgn_hip.h"
#include <cmath>
#include "awgn_math.hpp"

#pragma clang fp contract(off) // the arithmetic is pinned: every product and sum rounded on its own (the library is built -ffp-contract=off as well)

namespace dvbs2 {

std::string awgn_check(float sigma, int max_streams, int max_samples)
{
    if (!std::isfinite(sigma) || sigma < 0.0f) return "sigma must be finite and not negative";
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535)";
    if (max_samples < 1 || max_samples > (1 << 30)) return "max_samples out of range (1..2^30)";
    return "";
}

std::string awgn_sigma(double esn0_db, double es, int sps, float* sigma)
{
    if (!sigma) return "sigma is null";
    if (!std::isfinite(esn0_db)) return "esn0_db must be finite";
    if (!std::isfinite(es) || es <= 0.0) return "es must be finite and positive";
    if (sps < 1) return "sps must be at least 1";
    const double n0 = es / std::pow(10.0, esn0_db / 10.0);
    const float s = (float)std::sqrt(n0 * sps / 2.0);
    if (!std::isfinite(s)) return "esn0_db and es give a sigma that float32 cannot hold";
    *sigma = s;
    return "";
}

void awgn_words(uint64_t seed, uint64_t stream_id, int64_t index, uint32_t* wa_wb) { awgn_words_of(seed, stream_id, index, &wa_wb[0], &wa_wb[1]); }

void awgn_sample(uint64_t seed, uint64_t stream_id, int64_t index, float* re_im)
{
    uint32_t wa, wb;
    awgn_words_of(seed, stream_id, index, &wa, &wb);
    const AwgnPair n = awgn_noise(wa, wb);
    re_im[0] = n.re; re_im[1] = n.im;
}

namespace {

constexpr int kLanes = kAwgnTile / 2;

// native vectors: an access of 16 bytes stays one instruction
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// Workgroup (x, y): generator blocks [256 x, 256 x + 256) of row y, counted from the block that holds the call's first sample. Block j
// holds the samples i0 = 2 j - (first_index & 1) and i0 + 1 of the row; i0 == -1 (an odd start) and i0 + 1 == n (an odd end) are the
// half blocks. kWide: sample i0 of every row of in and out is 16-byte aligned. Nothing is read or written outside [0, n) of a row.
template <bool kWide, bool kIn>
__global__ __launch_bounds__(kLanes) void awgn_kernel(const v2f* in, long long in_stride, v2f* out, long long out_stride,
                                                      const float* __restrict__ sigmas, float sigma, uint64_t seed, uint64_t first_stream,
                                                      long long first_index, int n)
{
    const int row = blockIdx.y;
    const long long j = (long long)blockIdx.x * kLanes + threadIdx.x;
    const long long i0 = 2 * j - (first_index & 1);
    if (i0 >= n) return;
    const bool lo = i0 >= 0, hi = i0 + 1 < n;
    if (sigmas) sigma = sigmas[row];

    const AwgnWords w = awgn_block(seed, first_stream + (uint64_t)row, ((uint64_t)first_index >> 1) + (uint64_t)j);
    const AwgnPair n0 = awgn_noise(w.w[0], w.w[1]), n1 = awgn_noise(w.w[2], w.w[3]);

    v2f* dst = out + (long long)row * out_stride + i0;
    v4f x = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (kIn) {
        const v2f* src = in + (long long)row * in_stride + i0;
        if (kWide && lo && hi) x = *reinterpret_cast<const v4f*>(src);
        else {
            if (lo) x.xy = src[0];
            if (hi) x.zw = src[1];
        }
    }
    const AwgnPair y0 = kIn ? awgn_channel(AwgnPair{ x.x, x.y }, sigma, n0) : awgn_channel(sigma, n0);
    const AwgnPair y1 = kIn ? awgn_channel(AwgnPair{ x.z, x.w }, sigma, n1) : awgn_channel(sigma, n1);
    if (kWide && lo && hi) *reinterpret_cast<v4f*>(dst) = v4f{ y0.re, y0.im, y1.re, y1.im };
    else {
        if (lo) dst[0] = v2f{ y0.re, y0.im };
        if (hi) dst[1] = v2f{ y1.re, y1.im };
    }
}

} // namespace

AwgnHip::AwgnHip(uint64_t seed, float sigma, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device), seed_(seed)
{
    if (const std::string bad = awgn_check(sigma, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    sigma_ = sigma;
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
}

int AwgnHip::set_sigma(float sigma)
{
    call_err_ = {};
    if (const std::string bad = awgn_check(sigma, 1, 1); !bad.empty()) { call_err_.argument(bad); return -1; }
    sigma_ = sigma;
    return 0;
}

int AwgnHip::add_device(const float* d_in, int64_t in_stride, int n_samples, int n_streams, uint64_t first_stream, int64_t first_index,
                        const float* d_sigma, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_samples == 0 || n_streams == 0) return 0;
    const int odd = (int)(first_index & 1);
    // sample i0 of the full blocks is sample `odd` (mod 2) of a row: 16-byte aligned when the row's base plus 8 * odd is, in every row
    const bool many = n_streams > 1;
    auto wide_at = [&](const float* p, int64_t stride) { return (((uintptr_t)p >> 3) + odd) % 2 == 0 && (!many || (stride & 1) == 0); };
    const bool wide = wide_at(d_out, out_stride) && (!d_in || wide_at(d_in, in_stride));
    auto kernel = d_in ? (wide ? awgn_kernel<true, true> : awgn_kernel<false, true>) : (wide ? awgn_kernel<true, false> : awgn_kernel<false, false>);
    const long long blocks = ((long long)odd + n_samples + 1) / 2;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((blocks + kLanes - 1) / kLanes), (unsigned)n_streams), dim3(kLanes), 0, stream,
                       reinterpret_cast<const v2f*>(d_in), (long long)in_stride, reinterpret_cast<v2f*>(d_out), (long long)out_stride, d_sigma,
                       sigma_, seed_, first_stream, (long long)first_index, n_samples);
    return launched("awgn kernel launch");
}

} // namespace dvbs2
