// pfbch_hip.hip -- see pfbch_hip.h.
#include "pfbch_hip.h"
#include "fft_twiddles.h"
#include "stream_device.hpp"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off) // the arithmetic is pinned: a product, then an addition (the library is built -ffp-contract=off as well)

namespace dvbs2 {

int pfbch_log2(int n_chan)
{
    for (int t = kPfbchMinLog2; t <= kPfbchMaxLog2; t++)
        if (n_chan == 1 << t) return t;
    return -1;
}

int pfbch_geometry(int n_chan, int decim, int ntaps, int* history, int* delay_num, int* taps_per_branch)
{
    if (pfbch_log2(n_chan) < 0 || decim < 1 || decim > n_chan || ntaps < 1 || ntaps > kPfbchMaxTaps) return -1;
    if (history) *history = ntaps - 1;
    if (delay_num) *delay_num = ntaps - 1;
    if (taps_per_branch) *taps_per_branch = (ntaps + n_chan - 1) / n_chan;
    return 0;
}

int64_t pfbch_produce(int64_t position, int decim, int n_in)
{
    if (position < 0 || position > kPfbchMaxPosition || decim < 1 || decim > kPfbchMaxChan || n_in < 0 || n_in > kPfbchMaxSamples) return -1;
    const int64_t end = position + n_in;
    return (end + decim - 1) / decim - (position + decim - 1) / decim;
}

int pfbch_twiddles(int n_chan, float* out)
{
    if (pfbch_log2(n_chan) < 0 || !out) return -1;
    fft_twiddles(n_chan, out);
    return 0;
}

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLds = 80 * 1024; // bytes a block takes at most: two workgroups per CU
constexpr int kHistPerThread = (kPfbchMaxTaps - 1 + kThreads - 1) / kThreads;
constexpr int kRowOf = kPfbchMaxChan; // the device's table: the selection, then from here the row of every channel or -1

// Scratch segment of one output instant's M points: one pad element per 16 as in spectrum_hip.hip, and an odd length, so that lanes
// that differ in the instant alone (the row stores) meet different banks
__host__ __device__ constexpr int pad(int i) { return i + (i >> 4); }
__host__ __device__ constexpr int seg_len(int M) { return pad(M) | 1; }
constexpr int brev(int i, int T)
{
    int r = 0;
    for (int b = 0; b < T; b++) r |= ((i >> b) & 1) << (T - 1 - b);
    return r;
}
// M >= 32, two passes: 3 2, 3 3, 4 3, 4 4 stages
constexpr int first_pass_bits(int T) { return (T + 1) / 2; }

struct PfbGeom {
    int32_t D, ntaps, tile;
    int32_t cols;   // LDS columns, odd: consecutive rows of one column fall on different banks
    int32_t n_sel;
    int32_t r0;     // the call's first output sits on its input sample r0
    int32_t n0m;    // the counter at the call's start, mod M
    int32_t n_out;
};

size_t lds_bytes(int T, int decim, int ntaps, int tile, int* cols)
{
    const int M = 1 << T;
    const int slots = M + (ntaps - 1) + (tile - 1) * decim; // the span at most: the alignment, the history, the outputs' newest samples
    *cols = ((slots + M - 1) / M) | 1;
    const size_t scratch = T > kPfbchRegisterLog2 ? (size_t)(kPfbchBatchPoints >> T) * seg_len(M) * sizeof(float2) : 0;
    return (size_t)M * *cols * sizeof(float2) + (size_t)((ntaps + 1) & ~1) * sizeof(float) + scratch;
}

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

// Stages S0 + 1 .. S0 + RB of the nseg scratch segments, in place: spectrum_hip.hip's pass. A group is the 2^RB points that differ in
// bits S0 .. S0 + RB - 1 of their index; a lane holds one group in registers at a time.
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

// Block (blockIdx.x, blockIdx.y) writes the outputs [blockIdx.x * tile, + tile) of the call, those of them below n_out, for stream
// blockIdx.y and every selected channel. With `first` the call's input sample under the tile's first output, the tile needs the call's
// samples from first - H on (H = ntaps - 1). LDS slot s holds the call's sample i0 + s, i0 = first - H - a0, a0 = the residue mod M of
// the ABSOLUTE index of sample first - H: slot 0 is a multiple of M in absolute terms, so slot s sits at row s mod M, column s div M.
// Samples before the call come from the stream's history, those before the history (only slots below a0) are zeros and meet no tap.
// Nothing is read at or past n_in (the last output's newest sample is below it), nothing written at or past n_out, no slot at or past
// M * cols (the host's lds_bytes), no scratch point past the batch's segments.
template <int T>
__global__ __launch_bounds__(kThreads) void pfbch_kernel(const float2* __restrict__ in, long long in_stride, const float2* __restrict__ hist,
                                                         const float* __restrict__ taps, const float2* __restrict__ tw,
                                                         const int32_t* __restrict__ table, float2* __restrict__ out, long long out_stride, PfbGeom g)
{
    constexpr int M = 1 << T;
    extern __shared__ float2 lds[];
    const int tid = threadIdx.x, D = g.D, H = g.ntaps - 1, stream = blockIdx.y;
    const int o0 = blockIdx.x * g.tile;
    const int n_here = min(g.tile, g.n_out - o0); // >= 1: the grid has ceil(n_out / tile) columns
    const int first = g.r0 + o0 * D;
    const int a0 = (g.n0m + first - H) & (M - 1);
    const int i0 = first - H - a0;
    const int n_slots = a0 + H + (n_here - 1) * D + 1; // <= kPfbchSpan
    float* __restrict__ tp = reinterpret_cast<float*>(lds + M * g.cols);
    const float2* __restrict__ x = in + (long long)stream * in_stride;
    const float2* __restrict__ h0 = hist + (long long)stream * H;
#pragma unroll 4
    for (int s = tid; s < n_slots; s += kThreads) {
        const int i = i0 + s; // < n_in
        float2 z = make_float2(0.0f, 0.0f);
        if (i >= 0) z = x[i];
        else if (i >= -H) z = h0[i + H];
        lds[(s & (M - 1)) * g.cols + (s >> T)] = z;
    }
    for (int t = tid; t < g.ntaps; t += kThreads) tp[t] = taps[t];
    __syncthreads();

    // Output j of the tile has its newest sample in slot e = a0 + H + j D, row em = e mod M, column ec = e div M. Branch r takes the taps
    // p + q M, p = (em - r) mod M, against row r at column ec - (r > em) - q: whole for q < qfull, and one more where p < rem.
    const int qfull = g.ntaps >> T, rem = g.ntaps & (M - 1);
    float2* __restrict__ y = out + (long long)stream * g.n_sel * out_stride + o0;

    if constexpr (T <= kPfbchRegisterLog2) {
        for (int j0 = 0; j0 < n_here; j0 += kThreads) {
            const int j = min(j0 + tid, n_here - 1); // a lane past the tile's end repeats the last output and stores nothing
            const int e = a0 + H + j * D, em = e & (M - 1), ec = e >> T;
            v2f acc[M];
            int sa[M], ta[M];
#pragma unroll
            for (int r = 0; r < M; r++) {
                const int wrap = r > em ? 1 : 0;
                ta[r] = em - r + (wrap ? M : 0);
                sa[r] = r * g.cols + ec - wrap;
                acc[r] = v2f{ 0.0f, 0.0f };
            }
            for (int q = 0; q < qfull; q++) {
#pragma unroll
                for (int r = 0; r < M; r++) {
                    const float2 z = lds[sa[r] - q];
                    const float h = tp[ta[r] + (q << T)];
                    acc[r] = acc[r] + v2f{ z.x, z.y } * h;
                }
            }
            if (rem) {
#pragma unroll
                for (int r = 0; r < M; r++)
                    if (ta[r] < rem) {
                        const float2 z = lds[sa[r] - qfull];
                        const float h = tp[ta[r] + (qfull << T)];
                        acc[r] = acc[r] + v2f{ z.x, z.y } * h;
                    }
            }
            float2 v[M];
#pragma unroll
            for (int r = 0; r < M; r++) v[brev(r, T)] = make_float2(acc[r].x, acc[r].y);
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
            if (j0 + tid < n_here) {
#pragma unroll
                for (int c = 0; c < M; c++) {
                    const int row = table[kRowOf + c];
                    if (row >= 0) y[(long long)row * out_stride + j] = v[c];
                }
            }
        }
    } else {
        constexpr int B = kPfbchBatchPoints >> T, SEG = seg_len(M), U = 4, RB1 = first_pass_bits(T);
        float2* __restrict__ sc = reinterpret_cast<float2*>(tp + ((g.ntaps + 1) & ~1));
        for (int b0 = 0; b0 < n_here; b0 += B) {
            const int nb = min(B, n_here - b0), n_items = nb << T;
            for (int base = 0; base < n_items; base += kThreads * U) {
                v2f acc[U];
                int sa[U], ta[U], to[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int it = min(base + tid + kThreads * u, n_items - 1); // past the end: the last item again, not stored
                    const int jb = it >> T, r = it & (M - 1);
                    const int e = a0 + H + (b0 + jb) * D, em = e & (M - 1), ec = e >> T;
                    const int wrap = r > em ? 1 : 0;
                    ta[u] = em - r + (wrap ? M : 0);
                    sa[u] = r * g.cols + ec - wrap;
                    to[u] = jb * SEG + pad((int)(__brev((unsigned)r) >> (32 - T)));
                    acc[u] = v2f{ 0.0f, 0.0f };
                }
                for (int q = 0; q < qfull; q++) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const float2 z = lds[sa[u] - q];
                        const float h = tp[ta[u] + (q << T)];
                        acc[u] = acc[u] + v2f{ z.x, z.y } * h;
                    }
                }
                if (rem) {
#pragma unroll
                    for (int u = 0; u < U; u++)
                        if (ta[u] < rem) {
                            const float2 z = lds[sa[u] - qfull];
                            const float h = tp[ta[u] + (qfull << T)];
                            acc[u] = acc[u] + v2f{ z.x, z.y } * h;
                        }
                }
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (base + tid + kThreads * u < n_items) sc[to[u]] = make_float2(acc[u].x, acc[u].y);
            }
            __syncthreads();
            run_pass<T, 0, RB1>(sc, tw, nb);
            __syncthreads();
            run_pass<T, RB1, T - RB1>(sc, tw, nb);
            __syncthreads();
            // row i of the selection, consecutive lanes consecutive instants
            for (int it = tid; it < g.n_sel * nb; it += kThreads) {
                const int i = it / nb, jb = it - i * nb;
                y[(long long)i * out_stride + b0 + jb] = sc[jb * SEG + pad(table[i])];
            }
            __syncthreads(); // the next batch overwrites the segments
        }
    }
}

// One block per stream behind pfbch_kernel on the same HIP stream: roll_history over the call's raw samples. H <= 4095.
__global__ __launch_bounds__(kThreads) void pfbch_state_kernel(const float2* __restrict__ in, long long in_stride, float2* __restrict__ hist, int n_in, int H)
{
    const float2* __restrict__ x = in + (long long)blockIdx.x * in_stride;
    roll_history<kThreads, kHistPerThread>(hist + (long long)blockIdx.x * H, H, n_in, [&](long long j) { return x[j]; });
}

template <int T> hipError_t allow_lds() { return hipFuncSetAttribute((const void*)pfbch_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds); }

template <int T> void launch(dim3 grid, size_t lds, hipStream_t stream, const float2* in, long long in_stride, const float2* hist, const float* taps,
                             const float2* tw, const int32_t* table, float2* out, long long out_stride, const PfbGeom& g)
{
    hipLaunchKernelGGL(pfbch_kernel<T>, grid, dim3(kThreads), lds, stream, in, in_stride, hist, taps, tw, table, out, out_stride, g);
}

} // namespace

std::string PfbchHip::check_args(int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples)
{
    if (pfbch_log2(n_chan) < 0) return "n_chan must be a power of two in 2..256";
    if (decim < 1 || decim > n_chan) return "decim must be in 1..n_chan";
    if (ntaps < 1 || ntaps > kPfbchMaxTaps) return "ntaps must be in 1..4096";
    if (const std::string bad = check_taps(taps, ntaps, "taps"); !bad.empty()) return bad;
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535)";
    if (max_samples < 1 || max_samples > kPfbchMaxSamples) return "max_samples out of range (1..2^24)";
    return "";
}

std::string PfbchHip::check_channels(int n_chan, const int* list, int n_sel)
{
    if (n_sel < 1 || n_sel > n_chan) return "n_sel must be in 1..n_chan";
    if (!list) return "null list";
    bool seen[kPfbchMaxChan] = {};
    for (int i = 0; i < n_sel; i++) {
        if (list[i] < 0 || list[i] >= n_chan) return "list[" + std::to_string(i) + "] is not a channel";
        if (seen[list[i]]) return "list[" + std::to_string(i) + "] repeats a channel";
        seen[list[i]] = true;
    }
    return "";
}

PfbchHip::PfbchHip(int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = check_args(n_chan, decim, taps, ntaps, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    n_chan_ = n_chan; log2_ = pfbch_log2(n_chan); decim_ = decim; ntaps_ = ntaps; tile_ = pfbch_tile(n_chan, decim, ntaps);
    std::vector<int> all((size_t)n_chan);
    for (int c = 0; c < n_chan; c++) all[c] = c;
    set_channels(all.data(), n_chan);
    int cols = 0;
    if (lds_bytes(log2_, decim_, ntaps_, tile_, &cols) > (size_t)kMaxLds) { err_.argument("the tile rule exceeds the LDS budget"); return; } // (never: the constants)
    const std::vector<float> staged = fft_twiddles_staged(n_chan, log2_);
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the taps", alloc(&d_taps_, (size_t)ntaps_));
    HIP_OK_AS("hipMalloc of the twiddles", alloc(&d_twiddles_, (size_t)n_chan));
    HIP_OK_AS("hipMalloc of the histories", alloc_zeroed(&d_hist_, (size_t)max_streams * std::max(ntaps_ - 1, 1)));
    HIP_OK_AS("hipMalloc of the selection", alloc(&d_table_, (size_t)2 * kPfbchMaxChan));
    HIP_OK(hipMemcpy(d_taps_, taps, (size_t)ntaps_ * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_twiddles_, staged.data(), (size_t)n_chan * sizeof(float2), hipMemcpyHostToDevice));
    // The largest block is above the 64 KiB a kernel gets unasked. The attribute belongs to the kernel, not to the handle: always the cap
    HIP_OK(allow_lds<1>()); HIP_OK(allow_lds<2>()); HIP_OK(allow_lds<3>()); HIP_OK(allow_lds<4>());
    HIP_OK(allow_lds<5>()); HIP_OK(allow_lds<6>()); HIP_OK(allow_lds<7>()); HIP_OK(allow_lds<8>());
}

int PfbchHip::set_channels(const int* list, int n_sel)
{
    call_err_ = {};
    if (const std::string bad = check_channels(n_chan_, list, n_sel); !bad.empty()) { call_err_.argument(bad); return -1; }
    list_.assign(list, list + n_sel);
    table_.assign((size_t)2 * kPfbchMaxChan, -1);
    for (int i = 0; i < n_sel; i++) {
        table_[i] = list[i];
        table_[kRowOf + list[i]] = i;
    }
    table_dirty_ = true;
    return 0;
}

int PfbchHip::reset()
{
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipDeviceSynchronize());
    HIP_RET(zero(d_hist_));
    counter_ = 0;
    return 0;
}

int PfbchHip::process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_in == 0) return 0; // no output, and nothing moves
    const int64_t n_out = produce(n_in);
    if (n_out < 0) { call_err_.argument("the sample counter is exhausted"); return -1; }
    if (n_streams > 0) {
        // The selection is pageable host memory: for such a source hipMemcpyAsync returns once the runtime has taken its own copy of the
        // bytes (the API's rule for pageable transfers from host to device), so a set_channels right behind this call may rewrite table_.
        // The flag stays up until both launches were accepted: a call that fails behind the copy sends the same bytes again
        if (table_dirty_) HIP_RET(hipMemcpyAsync(d_table_, table_.data(), table_.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        const int D = decim_, H = ntaps_ - 1;
        const float2* in = reinterpret_cast<const float2*>(d_in);
        if (n_out > 0) {
            PfbGeom g = { D, ntaps_, tile_, 0, (int32_t)list_.size(), (int32_t)((D - counter_ % D) % D), (int32_t)(counter_ & (n_chan_ - 1)), (int32_t)n_out };
            const size_t lds = lds_bytes(log2_, D, ntaps_, tile_, &g.cols); // <= kMaxLds
            const dim3 grid((unsigned)((n_out + tile_ - 1) / tile_), (unsigned)n_streams);
            float2* out = reinterpret_cast<float2*>(d_out);
            switch (log2_) {
            case 1: launch<1>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            case 2: launch<2>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            case 3: launch<3>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            case 4: launch<4>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            case 5: launch<5>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            case 6: launch<6>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            case 7: launch<7>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            default: launch<8>(grid, lds, stream, in, in_stride, d_hist_, d_taps_, d_twiddles_, d_table_, out, out_stride, g); break;
            }
            if (launched("pfbch kernel launch")) return -1;
        }
        if (H > 0) {
            hipLaunchKernelGGL(pfbch_state_kernel, dim3(n_streams), dim3(kThreads), 0, stream, in, (long long)in_stride, d_hist_, n_in, H);
            if (launched("pfbch state kernel launch")) return -1;
        }
        table_dirty_ = false;
    }
    counter_ += n_in;
    return 0;
}

} // namespace dvbs2
