// agc_hip.hip -- see agc_hip.h.
#include "agc_hip.h"
#include <cmath>
#include <limits>
#include <vector>

#pragma clang fp contract(off) // the arithmetic is pinned: every product and sum rounded on its own (the library is built -ffp-contract=off as well)

namespace dvbs2 {

std::string agc_check(float rate, float reference, float gain, float max_gain)
{
    if (!std::isfinite(rate) || rate < 0.0f) return "rate must be finite and not negative";
    if (!std::isfinite(reference)) return "reference must be finite";
    if (!std::isfinite(gain)) return "gain must be finite";
    if (!std::isfinite(max_gain) || max_gain < 0.0f) return "max_gain must be finite and not negative (0: no cap)";
    return "";
}

int agc_lanes(int n_streams)
{
#ifdef DVBS2_AGC_LANES // kernel experiments (tools/build_variant.sh): one width for every batch
    return DVBS2_AGC_LANES;
#else
    for (int w = 8; w < 32; w *= 2)
        if ((n_streams + w - 1) / w <= 2048) return w;
    return 32;
#endif
}

namespace {

constexpr int kPitch = 2 * kAgcTile + 4; // floats per row of the sample tile: 4 dwords past a multiple of 64, rows stay 16-byte aligned
constexpr int kGainPitch = kAgcTile + 4; // floats per row of the gain tile: 4 dwords past a multiple of 32
constexpr int kRowChunks = kAgcTile / 2; // 16-byte pieces of a row of samples
constexpr int kGainChunks = kAgcTile / 4; // 16-byte pieces of a row of gains
static_assert((2 * kAgcTile) % 64 == 0 && 64 % kRowChunks == 0 && 64 % kGainChunks == 0, "the tile fixes the pitches and the lane -> piece map");

// native vectors: an access of 16 bytes stays one instruction (a float4 struct is taken apart where one branch fills it by halves)
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct AgcArgs {
    float rate, reference, cap; // cap: max_gain, +infinity for none (g > cap is then never true)
    int swap_iq, want_gain;
};

// one sample: returns the output and moves the gain on
__device__ __forceinline__ v2f agc_step(v2f x, float& g, const AgcArgs& p)
{
    const float yr = x.x * g, yi = x.y * g;
    const float m = sqrtf(yr * yr + yi * yi); // correctly rounded, denormals kept
    g = g + p.rate * (p.reference - m);
    if (g > p.cap) g = p.cap;
    return v2f{ yr, yi };
}

// Workgroup b = one wavefront: streams [b W, b W + W) of the call, lane l < W walks stream b W + l. kWide: every row of in, out and
// gain_out starts 16-byte aligned. Nothing is read or written past n samples of a stream or past n_streams streams.
template <int W, bool kWide>
__global__ __launch_bounds__(64) void agc_kernel(const v2f* in, long long in_stride, v2f* out, long long out_stride, float* gain_out,
                                                 long long gain_stride, float* __restrict__ state, int n, int n_streams, AgcArgs p)
{
    __shared__ __attribute__((aligned(16))) float tile[W * kPitch];
    __shared__ __attribute__((aligned(16))) float gains[W * kGainPitch];
    constexpr int kStage = W * kRowChunks / 64, kGainStage = W * kGainChunks / 64; // pieces a lane moves per tile
    const int lane = threadIdx.x, first = blockIdx.x * W;
    const int mine = first + lane;
    const bool walker = lane < W && mine < n_streams;
    float g = walker ? state[mine] : 0.0f;

    v4f stage[kStage];
    auto load_tile = [&](int base) { // samples [base, base + kAgcTile) of every row into registers
        const int n_here = min(kAgcTile, n - base);
#pragma unroll
        for (int j = 0; j < kStage; j++) {
            const int q = lane + 64 * j, r = first + q / kRowChunks, c = 2 * (q % kRowChunks);
            v4f v = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (r < n_streams && c < n_here) {
                const v2f* src = in + (long long)r * in_stride + base + c;
                if (kWide && c + 1 < n_here) v = *reinterpret_cast<const v4f*>(src);
                else {
                    v.xy = src[0];
                    if (c + 1 < n_here) v.zw = src[1];
                }
            }
            stage[j] = v;
        }
    };

    load_tile(0);
    for (int base = 0; base < n; base += kAgcTile) {
        const int n_here = min(kAgcTile, n - base);
#pragma unroll
        for (int j = 0; j < kStage; j++) {
            const int q = lane + 64 * j;
            v4f v = stage[j];
            if (p.swap_iq) v = v.yxwz;
            *reinterpret_cast<v4f*>(tile + (q / kRowChunks) * kPitch + 4 * (q % kRowChunks)) = v;
        }
        __syncthreads();
        if (base + kAgcTile < n) load_tile(base + kAgcTile); // in flight while the rows are walked

        if (walker) {
            float* row = tile + lane * kPitch;
            float* grow = gains + lane * kGainPitch;
            int i = 0;
            for (; i + 4 <= n_here; i += 4) {
                v4f a = *reinterpret_cast<v4f*>(row + 2 * i), b = *reinterpret_cast<v4f*>(row + 2 * i + 4);
                v4f gv;
                gv.x = g; a.xy = agc_step(a.xy, g, p);
                gv.y = g; a.zw = agc_step(a.zw, g, p);
                gv.z = g; b.xy = agc_step(b.xy, g, p);
                gv.w = g; b.zw = agc_step(b.zw, g, p);
                *reinterpret_cast<v4f*>(row + 2 * i) = a;
                *reinterpret_cast<v4f*>(row + 2 * i + 4) = b;
                if (p.want_gain) *reinterpret_cast<v4f*>(grow + i) = gv;
            }
            for (; i < n_here; i++) {
                v2f* x = reinterpret_cast<v2f*>(row + 2 * i);
                grow[i] = g;
                *x = agc_step(*x, g, p);
            }
        }
        __syncthreads();

#pragma unroll
        for (int j = 0; j < kStage; j++) {
            const int q = lane + 64 * j, r = first + q / kRowChunks, c = 2 * (q % kRowChunks);
            if (r < n_streams && c < n_here) {
                const v4f v = *reinterpret_cast<const v4f*>(tile + (q / kRowChunks) * kPitch + 2 * c);
                v2f* dst = out + (long long)r * out_stride + base + c;
                if (kWide && c + 1 < n_here) *reinterpret_cast<v4f*>(dst) = v;
                else {
                    dst[0] = v.xy;
                    if (c + 1 < n_here) dst[1] = v.zw;
                }
            }
        }
        if (p.want_gain) {
#pragma unroll
            for (int j = 0; j < kGainStage; j++) {
                const int q = lane + 64 * j, r = first + q / kGainChunks, c = 4 * (q % kGainChunks);
                if (r < n_streams && c < n_here) {
                    const v4f v = *reinterpret_cast<const v4f*>(gains + (q / kGainChunks) * kGainPitch + c);
                    float* dst = gain_out + (long long)r * gain_stride + base + c;
                    if (kWide && c + 3 < n_here) *reinterpret_cast<v4f*>(dst) = v;
                    else {
                        dst[0] = v.x;
                        if (c + 1 < n_here) dst[1] = v.y;
                        if (c + 2 < n_here) dst[2] = v.z;
                        if (c + 3 < n_here) dst[3] = v.w;
                    }
                }
            }
        }
        __syncthreads(); // the tile is read out before the next one is written over it
    }
    if (walker) state[mine] = g;
}

} // namespace

std::string AgcHip::check_args(float rate, float reference, float gain, float max_gain, int max_streams, int max_samples)
{
    if (const std::string bad = agc_check(rate, reference, gain, max_gain); !bad.empty()) return bad;
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535)";
    if (max_samples < 1 || max_samples > (1 << 30)) return "max_samples out of range (1..2^30)";
    return "";
}

AgcHip::AgcHip(float rate, float reference, float gain, float max_gain, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = check_args(rate, reference, gain, max_gain, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    rate_ = rate; reference_ = reference; gain0_ = gain; max_gain_ = max_gain;
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the gains", alloc(&d_state_, (size_t)max_streams_));
    const std::vector<float> g0((size_t)max_streams_, gain0_);
    HIP_OK(hipMemcpy(d_state_, g0.data(), g0.size() * sizeof(float), hipMemcpyHostToDevice));
}

int AgcHip::set_params(float rate, float reference, float max_gain)
{
    call_err_ = {};
    if (const std::string bad = agc_check(rate, reference, 0.0f, max_gain); !bad.empty()) { call_err_.argument(bad); return -1; }
    rate_ = rate; reference_ = reference; max_gain_ = max_gain;
    return 0;
}

int AgcHip::fill(int first, int count, float g)
{
    const std::vector<float> v((size_t)count, g);
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(hipMemcpy(d_state_ + first, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int AgcHip::reset()
{
    Entry on(*this);
    if (!on.ok) return -1;
    return fill(0, max_streams_, gain0_);
}

int AgcHip::set_gain(int stream_index, float g)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (stream_index < -1 || stream_index >= max_streams_) { call_err_.argument("stream index out of range"); return -1; }
    if (!std::isfinite(g)) { call_err_.argument("gain must be finite"); return -1; }
    return stream_index < 0 ? fill(0, max_streams_, g) : fill(stream_index, 1, g);
}

int AgcHip::state(float* gains, int n_streams)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (!gains) { call_err_.argument("gains is null"); return -1; }
    if (n_streams < 1 || n_streams > max_streams_) { call_err_.argument("n_streams out of range (1..max_streams)"); return -1; }
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(hipMemcpy(gains, d_state_, (size_t)n_streams * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int AgcHip::work_device(const float* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out, int64_t out_stride, float* d_gain,
                        int64_t gain_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_samples == 0 || n_streams == 0) return 0;
    const AgcArgs p = { rate_, reference_, max_gain_ > 0.0f ? max_gain_ : std::numeric_limits<float>::infinity(), swap_iq_ ? 1 : 0, d_gain ? 1 : 0 };
    const bool many = n_streams > 1; // a row starts 16-byte aligned when the base does and every stream starts at a multiple of 16 bytes
    const bool wide = ((uintptr_t)d_in & 15) == 0 && ((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_gain & 15) == 0 &&
                      (!many || ((in_stride & 1) == 0 && (out_stride & 1) == 0 && (!d_gain || (gain_stride & 3) == 0)));
    const int w = agc_lanes(n_streams);
    auto kernel = w == 8 ? (wide ? agc_kernel<8, true> : agc_kernel<8, false>)
                : w == 16 ? (wide ? agc_kernel<16, true> : agc_kernel<16, false>) : (wide ? agc_kernel<32, true> : agc_kernel<32, false>);
    hipLaunchKernelGGL(kernel, dim3((n_streams + w - 1) / w), dim3(64), 0, stream, reinterpret_cast<const v2f*>(d_in), (long long)in_stride,
                       reinterpret_cast<v2f*>(d_out), (long long)out_stride, d_gain, (long long)gain_stride, d_state_, n_samples, n_streams, p);
    return launched("agc kernel launch");
}

} // namespace dvbs2
