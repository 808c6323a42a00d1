// pfbsyn_hip.hip -- see pfbsyn_hip.h.
#include "pfbsyn_hip.h"
#include "fft_twiddles.h"
#include "stream_device.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off) // the arithmetic is pinned: a product, then an addition (the library is built -ffp-contract=off as well)

namespace dvbs2 {

int pfbsyn_log2(int n_chan)
{
    for (int t = kPfbsynMinLog2; t <= kPfbsynMaxLog2; t++)
        if (n_chan == 1 << t) return t;
    return -1;
}

int pfbsyn_geometry(int n_chan, int interp, int ntaps, int* tail, int* delay_num, int* taps_per_phase)
{
    if (pfbsyn_log2(n_chan) < 0 || interp < 1 || interp > n_chan || ntaps < 1 || ntaps > kPfbsynMaxTaps) return -1;
    if (tail) *tail = std::max(ntaps - interp, 0);
    if (delay_num) *delay_num = ntaps - 1;
    if (taps_per_phase) *taps_per_phase = (ntaps + interp - 1) / interp;
    return 0;
}

int64_t pfbsyn_advance(int64_t position, int n_in)
{
    if (position < 0 || position > kPfbsynMaxPosition || n_in < 0 || n_in > kPfbsynMaxSamples) return -1;
    return position + n_in > kPfbsynMaxPosition ? -1 : position + n_in;
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLds = kPfbsynSpanLong * (int)sizeof(float2) + kPfbsynMaxTaps * (int)sizeof(float); // 120 KiB: the long store and every tap

// An instant's M points in the store: one pad element per 16 as in spectrum_hip.hip and pfbch_hip.hip, and an odd length, so that lanes
// that differ in the instant alone meet different banks
__host__ __device__ constexpr int pad(int i) { return i + (i >> 4); }
__host__ __device__ constexpr int seg_len(int M) { return pad(M) | 1; }
static_assert(seg_len(2) == pfbsyn_seg_len(2) && seg_len(16) == pfbsyn_seg_len(16) && seg_len(256) == pfbsyn_seg_len(256), "the tile rule counts the store's rows");
constexpr int brev(int i, int T)
{
    int r = 0;
    for (int b = 0; b < T; b++) r |= ((i >> b) & 1) << (T - 1 - b);
    return r;
}
// M >= 32, two passes: 3 2, 3 3, 4 3, 4 4 stages
constexpr int first_pass_bits(int T) { return (T + 1) / 2; }

struct SynGeom {
    int32_t L, ntaps, q, tile;
    int32_t rows;   // instants the store has room for: tile + q - 1
    int32_t n_sel;
    int32_t n0m;    // the absolute index of the call's first output, mod M
    int32_t n_in, tail;
};

size_t lds_bytes(int M, int ntaps, int rows) { return (size_t)rows * seg_len(M) * sizeof(float2) + (size_t)((ntaps + 1) & ~1) * sizeof(float); }

// The stage code of pfbch_hip.hip, this file's own copy (notes/shared_stream_device.md): to be kept equal by hand.
// one butterfly stage behind the first over the R points of v: index j pairs with j + half, W from w[j mod half]
template <int R> __device__ inline void butterflies(float2* v, const float2* w, int half)
{
#pragma unroll
    for (int j = 0; j < R; j++) {
        if (j & half) continue;
        const float2 a = v[j], b = v[j + half], W = w[j & (half - 1)];
        const float tr = W.x * b.x - W.y * b.y, ti = W.x * b.y + W.y * b.x;
        v[j] = make_float2(a.x + tr, a.y + ti);
        v[j + half] = make_float2(a.x - tr, a.y - ti);
    }
}
template <int R> __device__ inline void first_stage(float2* v)
{
#pragma unroll
    for (int j = 0; j < R; j += 2) {
        const float2 a = v[j], b = v[j + 1];
        v[j] = make_float2(a.x + b.x, a.y + b.y);
        v[j + 1] = make_float2(a.x - b.x, a.y - b.y);
    }
}

// Stages S0 + 1 .. S0 + RB of the nseg store segments, in place. A group is the 2^RB points that differ in bits S0 .. S0 + RB - 1 of
// their index; a lane holds one group in registers at a time.
template <int T, int S0, int RB> __device__ inline void run_pass(float2* __restrict__ sc, const float2* __restrict__ tw, int nseg)
{
    constexpr int N = 1 << T, R = 1 << RB, G = N >> RB, SEG = seg_len(N);
    for (int gi = threadIdx.x; gi < nseg * G; gi += kThreads) {
        const int sl = gi / G, g = gi % G; // (powers of two)
        const int low = g & ((1 << S0) - 1), high = g >> S0;
        const int base = low + (high << (S0 + RB));
        float2* __restrict__ seg = sc + sl * SEG;
        float2 v[R];
#pragma unroll
        for (int j = 0; j < R; j++) v[j] = seg[pad(base + (j << S0))];
#pragma unroll
        for (int q = 1; q <= RB; q++) {
            constexpr int kHalfMax = R / 2 > 0 ? R / 2 : 1;
            const int half = 1 << (q - 1);
            if (S0 == 0 && q == 1) {
                first_stage<R>(v);
            } else {
                // stage s = S0 + q takes entry k 2^(T - s) of the table, k = low + jj 2^S0: entry 2^(s-1) - 1 + k of the copy in stage order
                float2 w[kHalfMax];
#pragma unroll
                for (int jj = 0; jj < half; jj++) w[jj] = tw[((1 << (S0 + q - 1)) - 1) + low + (jj << S0)]; // below M - 1
                butterflies<R>(v, w, half);
            }
        }
#pragma unroll
        for (int j = 0; j < R; j++) seg[pad(base + (j << S0))] = v[j];
    }
}

// Block (blockIdx.x, blockIdx.y) owns the instants [m0, m0 + n_here) of the call, m0 = blockIdx.x * tile, for stream blockIdx.y; the
// instants run to n_in + q - 1: those at and past n_in do not exist, their outputs are the new tail. The store holds the transformed
// instants [s_lo, s_hi) = [max(m0 - (q - 1), 0), min(m0 + n_here, n_in)), at least one and at most tile + q - 1 = g.rows. Output i of the
// call (absolute k0 L + i), m0 L <= i < (m0 + n_here) L and i < n_in L + tail, takes the instants m1 - j, m1 = i div L, for the j of its
// taps with 0 <= m1 - j < n_in: all of them at or above m1 - (q - 1) >= s_lo and below s_hi. Nothing is read from the rows at or past
// n_in, nothing written to `out` at or past n_in L nor to `tnext` at or past tail, no store row at or past ns, no tap at or past ntaps.
// The store holds what the graph returns, (v.im, v.re): the sums are formed on that and exchanged where they leave or enter.
template <int T>
__global__ __launch_bounds__(kThreads) void pfbsyn_kernel(const float2* __restrict__ in, long long in_stride, const float2* __restrict__ tail,
                                                          float2* __restrict__ tail_next, const float* __restrict__ taps,
                                                          const float2* __restrict__ tw, const int32_t* __restrict__ table,
                                                          float2* __restrict__ out, long long out_stride, SynGeom g)
{
    constexpr int M = 1 << T, SEG = seg_len(M);
    extern __shared__ float2 lds[];
    const int tid = threadIdx.x, L = g.L, q = g.q, stream = blockIdx.y;
    const int m0 = blockIdx.x * g.tile;
    const int n_here = min(g.tile, g.n_in + q - 1 - m0); // >= 1: the grid has ceil((n_in + q - 1) / tile) columns
    const int s_lo = max(m0 - (q - 1), 0), s_hi = min(m0 + n_here, g.n_in), ns = s_hi - s_lo;
    float* __restrict__ tp = reinterpret_cast<float*>(lds + g.rows * SEG);
    const float2* __restrict__ x = in + (long long)stream * g.n_sel * in_stride + s_lo;
    for (int t = tid; t < g.ntaps; t += kThreads) tp[t] = taps[t];

    if constexpr (T <= kPfbsynRegisterLog2) {
        for (int inst = tid; inst < ns; inst += kThreads) {
            float2 v[M];
#pragma unroll
            for (int c = 0; c < M; c++) {
                const int row = table[c]; // uniform: a scalar load
                float2 a = make_float2(0.0f, 0.0f);
                if (row >= 0) a = x[(long long)row * in_stride + inst];
                v[brev(c, T)] = make_float2(a.y, a.x);
            }
            first_stage<M>(v);
#pragma unroll
            for (int s = 2; s <= T; s++) {
                constexpr int kHalfMax = M / 2;
                const int half = 1 << (s - 1);
                float2 w[kHalfMax];
#pragma unroll
                for (int k = 0; k < half; k++) w[k] = tw[half - 1 + k]; // uniform: scalar loads
                butterflies<M>(v, w, half);
            }
#pragma unroll
            for (int r = 0; r < M; r++) lds[inst * SEG + pad(r)] = v[r];
        }
        __syncthreads();
    } else {
        constexpr int RB1 = first_pass_bits(T);
        // for one channel consecutive lanes read consecutive instants of its row and write an odd segment length apart
        for (int it = tid; it < ns * M; it += kThreads) {
            const int c = it / ns, inst = it - c * ns;
            const int row = table[c];
            float2 a = make_float2(0.0f, 0.0f);
            if (row >= 0) a = x[(long long)row * in_stride + inst];
            lds[inst * SEG + pad((int)(__brev((unsigned)c) >> (32 - T)))] = make_float2(a.y, a.x);
        }
        __syncthreads();
        run_pass<T, 0, RB1>(lds, tw, ns);
        __syncthreads();
        run_pass<T, RB1, T - RB1>(lds, tw, ns);
        __syncthreads();
    }

    const int n_out = g.n_in * L;                           // <= 2^28
    const int i_end = min((m0 + n_here) * L, n_out + g.tail);
    const int p_last = g.ntaps - 1 - (q - 1) * L;           // >= 0: the phases up to it have q taps, those above q - 1
    const float2* __restrict__ t_old = tail + (long long)stream * g.tail;
    float2* __restrict__ t_new = tail_next + (long long)stream * g.tail;
    float2* __restrict__ y = out + (long long)stream * out_stride;
    for (int i = m0 * L + tid; i < i_end; i += kThreads) {
        const int m1 = i / L, p = i - m1 * L, r = (g.n0m + i) & (M - 1);
        const int j_hi = min(p <= p_last ? q - 1 : q - 2, m1); // the oldest term: its tap exists and its instant is not before the call
        const int j_lo = max(m1 - (g.n_in - 1), 0);            // the newest: its instant exists
        v2f acc = v2f{ 0.0f, 0.0f };
        if (i < g.tail) {
            const float2 t = t_old[i];
            acc = v2f{ t.y, t.x };
        }
        const int at = (m1 - s_lo) * SEG + pad(r);
#pragma unroll 4
        for (int j = j_hi; j >= j_lo; j--) {
            const float2 z = lds[at - j * SEG];
            const float h = tp[p + j * L];
            acc = acc + v2f{ z.x, z.y } * h;
        }
        const float2 sum = make_float2(acc.y, acc.x);
        if (i < n_out) y[i] = sum;
        else t_new[i - n_out] = sum;
    }
}

// Behind pfbsyn_kernel on the same HIP stream: the tails the call left, n of them over all its streams, take the place of the old ones.
__global__ __launch_bounds__(kThreads) void pfbsyn_state_kernel(const float2* __restrict__ tail_next, float2* __restrict__ tail, long long n)
{
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) tail[i] = tail_next[i];
}

template <int T> hipError_t allow_lds() { return hipFuncSetAttribute((const void*)pfbsyn_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds); }

template <int T> void launch(dim3 grid, size_t lds, hipStream_t stream, const float2* in, long long in_stride, const float2* tail, float2* tail_next,
                             const float* taps, const float2* tw, const int32_t* table, float2* out, long long out_stride, const SynGeom& g)
{
    hipLaunchKernelGGL(pfbsyn_kernel<T>, grid, dim3(kThreads), lds, stream, in, in_stride, tail, tail_next, taps, tw, table, out, out_stride, g);
}

} // namespace

std::string PfbsynHip::check_args(int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples)
{
    if (pfbsyn_log2(n_chan) < 0) return "n_chan must be a power of two in 2..256";
    if (interp < 1 || interp > n_chan) return "interp must be in 1..n_chan";
    if (ntaps < 1 || ntaps > kPfbsynMaxTaps) return "ntaps must be in 1..4096";
    if (const std::string bad = check_taps(taps, ntaps, "taps"); !bad.empty()) return bad;
    if (n_chan * ((ntaps + interp - 1) / interp) > kPfbsynMaxProduct) return "n_chan * ceil(ntaps / interp) must not exceed 8192";
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535)";
    if (max_samples < 1 || max_samples > kPfbsynMaxSamples) return "max_samples out of range (1..2^24)";
    if ((int64_t)max_samples * interp > kPfbsynMaxOut) return "max_samples * interp must not exceed 2^28";
    return "";
}

std::string PfbsynHip::check_channels(int n_chan, const int* list, int n_sel)
{
    if (n_sel < 1 || n_sel > n_chan) return "n_sel must be in 1..n_chan";
    if (!list) return "null list";
    bool seen[kPfbsynMaxChan] = {};
    for (int i = 0; i < n_sel; i++) {
        if (list[i] < 0 || list[i] >= n_chan) return "list[" + std::to_string(i) + "] is not a channel";
        if (seen[list[i]]) return "list[" + std::to_string(i) + "] repeats a channel";
        seen[list[i]] = true;
    }
    return "";
}

PfbsynHip::PfbsynHip(int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = check_args(n_chan, interp, taps, ntaps, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    n_chan_ = n_chan; log2_ = pfbsyn_log2(n_chan); interp_ = interp; ntaps_ = ntaps;
    pfbsyn_geometry(n_chan, interp, ntaps, &tail_, nullptr, &q_);
    tile_ = pfbsyn_tile(n_chan, interp, ntaps);
    std::vector<int> all((size_t)n_chan);
    for (int c = 0; c < n_chan; c++) all[c] = c;
    set_channels(all.data(), n_chan);
    if (tile_ < 1 || lds_bytes(n_chan_, ntaps_, tile_ + q_ - 1) > (size_t)kMaxLds) { err_.argument("the tile rule exceeds the LDS budget"); return; } // (never: the constants)
    const std::vector<float> staged = fft_twiddles_staged(n_chan, log2_);
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the taps", alloc(&d_taps_, (size_t)ntaps_));
    HIP_OK_AS("hipMalloc of the twiddles", alloc(&d_twiddles_, (size_t)n_chan));
    HIP_OK_AS("hipMalloc of the tails", alloc_zeroed(&d_tail_, (size_t)2 * max_streams * std::max(tail_, 1)));
    HIP_OK_AS("hipMalloc of the selection", alloc(&d_table_, (size_t)kPfbsynMaxChan));
    HIP_OK(hipMemcpy(d_taps_, taps, (size_t)ntaps_ * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_twiddles_, staged.data(), (size_t)n_chan * sizeof(float2), hipMemcpyHostToDevice));
    // The largest block is above the 64 KiB a kernel gets unasked. The attribute belongs to the kernel, not to the handle: always the cap
    HIP_OK(allow_lds<1>()); HIP_OK(allow_lds<2>()); HIP_OK(allow_lds<3>()); HIP_OK(allow_lds<4>());
    HIP_OK(allow_lds<5>()); HIP_OK(allow_lds<6>()); HIP_OK(allow_lds<7>()); HIP_OK(allow_lds<8>());
}

int PfbsynHip::set_channels(const int* list, int n_sel)
{
    call_err_ = {};
    if (const std::string bad = check_channels(n_chan_, list, n_sel); !bad.empty()) { call_err_.argument(bad); return -1; }
    list_.assign(list, list + n_sel);
    table_.assign((size_t)kPfbsynMaxChan, -1);
    for (int i = 0; i < n_sel; i++) table_[list[i]] = i;
    table_dirty_ = true;
    return 0;
}

int PfbsynHip::reset()
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(zero(d_tail_));
    counter_ = 0;
    return 0;
}

int PfbsynHip::process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_in == 0) return 0; // no output, and nothing moves
    if (produce(n_in) < 0) { call_err_.argument("the sample counter is exhausted"); return -1; }
    if (n_streams > 0) {
        // The selection is pageable host memory: for such a source hipMemcpyAsync returns once the runtime has taken its own copy of the
        // bytes, so a set_channels right behind this call may rewrite table_. The flag stays up until both launches were accepted
        if (table_dirty_) HIP_RET(hipMemcpyAsync(d_table_, table_.data(), table_.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        const SynGeom g = { interp_, ntaps_, q_, tile_, tile_ + q_ - 1, (int32_t)list_.size(), (int32_t)((counter_ * interp_) & (n_chan_ - 1)), n_in, tail_ };
        const size_t lds = lds_bytes(n_chan_, ntaps_, g.rows); // <= kMaxLds
        const dim3 grid((unsigned)((n_in + q_ - 1 + tile_ - 1) / tile_), (unsigned)n_streams);
        const float2* in = reinterpret_cast<const float2*>(d_in);
        float2* out = reinterpret_cast<float2*>(d_out);
        float2* next = d_tail_ + (size_t)max_streams_ * std::max(tail_, 1);
        switch (log2_) {
        case 1: launch<1>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        case 2: launch<2>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        case 3: launch<3>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        case 4: launch<4>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        case 5: launch<5>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        case 6: launch<6>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        case 7: launch<7>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        default: launch<8>(grid, lds, stream, in, in_stride, d_tail_, next, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
        }
        if (launched("pfbsyn kernel launch")) return -1;
        if (tail_ > 0) {
            const long long n = (long long)n_streams * tail_;
            const unsigned blocks = (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, 1024);
            hipLaunchKernelGGL(pfbsyn_state_kernel, dim3(blocks), dim3(kThreads), 0, stream, next, d_tail_, n);
            if (launched("pfbsyn state kernel launch")) return -1;
        }
        table_dirty_ = false;
    }
    counter_ += n_in;
    return 0;
}

} // namespace dvbs2
