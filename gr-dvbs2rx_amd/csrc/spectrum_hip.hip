// spectrum_hip.hip -- see spectrum_hip.h.
#include "spectrum_hip.h"
#include "fft_twiddles.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off) // the arithmetic is pinned: products, then an addition (the library is built -ffp-contract=off as well)

namespace dvbs2 {

static int spectrum_log2(int nfft)
{
    for (int t = kSpectrumMinLog2; t <= kSpectrumMaxLog2; t++)
        if (nfft == 1 << t) return t;
    return -1;
}

int spectrum_geometry(int nfft, int hop, int avg, int n_in, int* n_seg, int* n_rows, int* used_samples)
{
    if (spectrum_log2(nfft) < 0 || hop < 1 || hop > kSpectrumMaxHop || avg < 0 || n_in < 0 || n_in > kSpectrumMaxSamples) return -1;
    const int seg = n_in >= nfft ? (n_in - nfft) / hop + 1 : 0;
    const int rows = avg > 0 ? seg / avg : (seg > 0 ? 1 : 0);
    const int used_seg = avg > 0 ? rows * avg : seg; // <= seg
    if (n_seg) *n_seg = seg;
    if (n_rows) *n_rows = rows;
    if (used_samples) *used_samples = used_seg > 0 ? (used_seg - 1) * hop + nfft : 0; // <= n_in
    return 0;
}

int spectrum_window(int kind, int nfft, float* out)
{
    if (spectrum_log2(nfft) < 0 || kind < kSpectrumRect || kind > kSpectrumBlackmanHarris || !out) return -1;
    for (int n = 0; n < nfft; n++) {
        const double x = 2.0 * M_PI * n / nfft;
        double w = 1.0;
        if (kind == kSpectrumHann) w = 0.5 - 0.5 * std::cos(x);
        else if (kind == kSpectrumHamming) w = 0.54 - 0.46 * std::cos(x);
        else if (kind == kSpectrumBlackmanHarris) w = 0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2.0 * x) - 0.01168 * std::cos(3.0 * x);
        out[n] = (float)w;
    }
    return 0;
}

int spectrum_twiddles(int nfft, float* out)
{
    if (spectrum_log2(nfft) < 0 || !out) return -1;
    fft_twiddles(nfft, out);
    return 0;
}

double spectrum_window_power(const float* window, int nfft)
{
    double s = 0.0;
    for (int n = 0; n < nfft; n++) s += (double)window[n] * (double)window[n];
    return s;
}

namespace {

constexpr int kThreads = 256;

// LDS position of point i of a segment: one pad element per 16, so that the 8 or 16 consecutive points a lane holds in the first pass
// start on different banks from lane to lane, and so do the runs of 16 lanes of the passes behind it
__host__ __device__ constexpr int pad(int i) { return i + (i >> 4); }
// The pass plan of nfft = 2^T: ceil(T / 4) passes of 3 or 4 stages (T = 6: 3 3, 7: 4 3, 8: 4 4, 9: 3 3 3, 10: 4 3 3, 11: 4 4 3,
// 12: 4 4 4, 13: 4 3 3 3)
constexpr int n_passes(int T) { return (T + 3) / 4; }
constexpr int pass_bits(int T, int i) { return T / n_passes(T) + (i < T % n_passes(T) ? 1 : 0); }
constexpr int last_pass_bits(int T) { return pass_bits(T, n_passes(T) - 1); }
// segments of a chunk that run side by side, so that every pass has a group for (nearly) every lane
constexpr int side_by_side(int T) { return T <= 8 ? kSpectrumChunk : T == 9 ? 4 : T == 10 ? 2 : 1; }
constexpr size_t lds_bytes(int T)
{
    const int ns = side_by_side(T);
    return (size_t)ns * pad(1 << T) * sizeof(float2) + (ns > 1 ? (size_t)ns * (1 << T) * sizeof(float) : 0);
}

struct SpecArgs {
    const float2* in; long long in_stride;
    const float* window;
    const float2* tw;  // the table in stage order: for stage s = 1..t its 2^(s-1) entries k 2^(t - s) of the table, k ascending
    float* partial;    // chunk sums [workgroup][nfft], bins in natural order (not used when direct)
    float* out; long long out_stride;
    int hop, n_rows, cpr, row_segs; // cpr: chunks per row; row_segs: segments per row
    int shift_mask;    // nfft / 2 when shifted, else 0: bin k is written at k ^ shift_mask
    int direct;        // a row is one chunk: the kernel scales and writes the row itself
    float scale;
};

// Stages S0 + 1 .. S0 + RB of the `nseg` segments in LDS. A group is the R = 2^RB points that differ in bits S0 .. S0 + RB - 1 of
// their index; a lane holds one group in registers, runs the RB stages on it and puts it back. In the last pass (S0 + RB == T) the
// powers stay with the lane (NS == 1: acc[m R + j] is bin g + j 2^S0 of the lane's m-th group g = thread + 256 m) or go to pw
// (NS > 1), where the caller adds them in segment order.
template <int T, int S0, int RB, int NS, bool LAST>
__device__ inline void run_pass(float2* __restrict__ lds, float* __restrict__ pw, const float2* __restrict__ tw, int nseg, float* acc)
{
    constexpr int N = 1 << T, R = 1 << RB, G = N >> RB, SEG = pad(N);
    constexpr int ITER = (NS * G + kThreads - 1) / kThreads;
    // (only the last pass needs m at compile time, for the registers of acc; one group at a time keeps the others' registers low)
    constexpr int UNROLL = LAST ? ITER : 1;
#pragma unroll UNROLL
    for (int m = 0; m < ITER; m++) {
        const int gi = threadIdx.x + m * kThreads;
        const int sl = gi / G, g = gi % G; // (powers of two)
        if (gi < NS * G && sl < nseg) {
            const int low = g & ((1 << S0) - 1), high = g >> S0;
            const int base = low + (high << (S0 + RB));
            float2* __restrict__ seg = lds + sl * SEG;
            float2 v[R];
#pragma unroll
            for (int j = 0; j < R; j++) v[j] = seg[pad(base + (j << S0))];
#pragma unroll
            for (int q = 1; q <= RB; q++) {
                const int half = 1 << (q - 1);
                if (S0 == 0 && q == 1) { // stage 1: no product
#pragma unroll
                    for (int j = 0; j < R; j += 2) {
                        const float2 a = v[j], b = v[j + 1];
                        v[j] = make_float2(a.x + b.x, a.y + b.y);
                        v[j + 1] = make_float2(a.x - b.x, a.y - b.y);
                    }
                } else {
                    // stage s = S0 + q takes entry k 2^(T - s) of the table, k = low + jj 2^S0 < 2^(s-1): entry 2^(s-1) - 1 + k of the
                    // copy in stage order, where consecutive lanes read consecutive entries
                    float2 w[R / 2];
#pragma unroll
                    for (int jj = 0; jj < half; jj++) w[jj] = tw[((1 << (S0 + q - 1)) - 1) + low + (jj << S0)]; // below nfft - 1
#pragma unroll
                    for (int j = 0; j < R; j++) {
                        if (j & half) continue;
                        const float2 a = v[j], b = v[j + half], W = w[j & (half - 1)];
                        const float tr = W.x * b.x - W.y * b.y, ti = W.x * b.y + W.y * b.x;
                        v[j] = make_float2(a.x + tr, a.y + ti);
                        v[j + half] = make_float2(a.x - tr, a.y - ti);
                    }
                }
            }
            if (!LAST) {
#pragma unroll
                for (int j = 0; j < R; j++) seg[pad(base + (j << S0))] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const float p = v[j].x * v[j].x + v[j].y * v[j].y;
                    if (NS == 1) acc[m * R + j] = acc[m * R + j] + p;
                    else pw[sl * N + base + (j << S0)] = p; // (the last pass: high == 0, base == g)
                }
            }
        }
    }
}

template <int T, int I, int S0, int NS>
__device__ inline void run_passes(float2* __restrict__ lds, float* __restrict__ pw, const float2* __restrict__ tw, int nseg, float* acc)
{
    constexpr int RB = pass_bits(T, I);
    constexpr bool LAST = I == n_passes(T) - 1;
    static_assert(!LAST || S0 + RB == T, "the passes cover the stages");
    run_pass<T, S0, RB, NS, LAST>(lds, pw, tw, nseg, acc);
    if constexpr (!LAST) {
        __syncthreads();
        run_passes<T, I + 1, S0 + RB, NS>(lds, pw, tw, nseg, acc);
    }
}

// Workgroup blockIdx.x = (stream n_rows + row) cpr + chunk adds the powers of segments [chunk 16, + n_here) of its row. Reads stay
// below the row's last sample (the host's geometry), writes within the workgroup's nfft floats of the scratch buffer or of the row.
// The second launch bound: at 8192 the LDS leaves room for two workgroups per CU, two waves per SIMD, and the registers must not bind
// before it (without the bound the compiler takes 256 and more). A bound of four waves at 1024..4096 spills; they stay as compiled.
template <int T>
__global__ __launch_bounds__(kThreads, T == 13 ? 2 : 1) void spectrum_kernel(SpecArgs a)
{
    constexpr int N = 1 << T, NS = side_by_side(T), SEG = pad(N), ACC = N >= kThreads ? N / kThreads : 1;
    extern __shared__ float2 lds[];
    float* pw = reinterpret_cast<float*>(lds + NS * SEG);
    const int tid = threadIdx.x;
    const unsigned blk = blockIdx.x;
    const int chunk = (int)(blk % (unsigned)a.cpr);
    const unsigned rest = blk / (unsigned)a.cpr;
    const int row = (int)(rest % (unsigned)a.n_rows), stream = (int)(rest / (unsigned)a.n_rows);
    const int first = chunk * kSpectrumChunk;                    // in the row
    const int n_here = min(kSpectrumChunk, a.row_segs - first); // >= 1
    const float2* __restrict__ x = a.in + (long long)stream * a.in_stride + ((long long)row * a.row_segs + first) * a.hop;

    float acc[ACC];
#pragma unroll
    for (int i = 0; i < ACC; i++) acc[i] = 0.0f;

    for (int s0 = 0; s0 < n_here; s0 += NS) {
        const int nseg = min(NS, n_here - s0);
        // The windowed samples to their bit-reversed places. A lane takes sample n = a + 4 c + (N / 16) b of thread index a + 4 b + 64 c:
        // runs of four samples (32 bytes) from memory, and the 16 values of b, the top bits of n, are the low bits of the place.
#pragma unroll 4
        for (int m = 0; m < NS * N / kThreads; m++) {
            const int L = tid + m * kThreads, sl = L >> T, Ls = L & (N - 1);
            const int n = (Ls & 3) + ((Ls >> 6) << 2) + (((Ls >> 2) & 15) << (T - 4));
            if (sl < nseg) {
                const float2 v = x[(long long)(s0 + sl) * a.hop + n];
                const float w = a.window[n];
                lds[sl * SEG + pad((int)(__brev((unsigned)n) >> (32 - T)))] = make_float2(v.x * w, v.y * w);
            }
        }
        __syncthreads();
        run_passes<T, 0, 0, NS>(lds, pw, a.tw, nseg, acc);
        if constexpr (NS > 1) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < ACC; m++) {
                const int b = tid + m * kThreads;
                if (b < N)
                    for (int sl = 0; sl < nseg; sl++) acc[m] = acc[m] + pw[sl * N + b];
            }
        }
        __syncthreads(); // the next segments overwrite what this pass read
    }

    float* __restrict__ part = a.partial + (long long)blk * N;
    float* __restrict__ rowp = a.out + (long long)stream * a.out_stride + (long long)row * N;
    constexpr int RL = 1 << last_pass_bits(T), S0L = T - last_pass_bits(T);
#pragma unroll
    for (int i = 0; i < ACC; i++) {
        // NS == 1: acc[m RL + j] is bin thread + 256 m + j 2^S0L; else acc[m] is bin thread + 256 m
        const int bin = NS == 1 ? tid + (i / RL) * kThreads + ((i % RL) << S0L) : tid + i * kThreads;
        if (bin < N) {
            if (a.direct) rowp[bin ^ a.shift_mask] = acc[i] * a.scale;
            else part[bin] = acc[i];
        }
    }
}

// Behind spectrum_kernel on the same HIP stream where a row has several chunks: block (stream n_rows + row, bins / 64) adds the row's
// chunk sums in ascending order onto +0.0f, scales and writes. One wavefront per block: a long row of one stream still meets many CUs.
constexpr int kFinishThreads = 64;
__global__ __launch_bounds__(kFinishThreads) void spectrum_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, long long out_stride,
                                                                   int N, int n_rows, int cpr, int shift_mask, float scale)
{
    const int bin = blockIdx.y * kFinishThreads + threadIdx.x;
    if (bin >= N) return;
    const int row = (int)(blockIdx.x % (unsigned)n_rows), stream = (int)(blockIdx.x / (unsigned)n_rows);
    const float* __restrict__ p = partial + (long long)blockIdx.x * cpr * N + bin;
    float s = 0.0f;
    int c = 0;
    for (; c + 16 <= cpr; c += 16) { // sixteen loads in flight, then their additions in order
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = p[(long long)(c + k) * N];
#pragma unroll
        for (int k = 0; k < 16; k++) s = s + v[k];
    }
    for (; c < cpr; c++) s = s + p[(long long)c * N];
    out[(long long)stream * out_stride + (long long)row * N + (bin ^ shift_mask)] = s * scale;
}

template <int T> void launch(const SpecArgs& a, unsigned blocks, hipStream_t stream)
{
    hipLaunchKernelGGL(spectrum_kernel<T>, dim3(blocks), dim3(kThreads), lds_bytes(T), stream, a);
}

} // namespace

std::string SpectrumHip::check_args(int nfft, int hop, int avg, const float* window, int max_streams, int max_samples)
{
    if (spectrum_log2(nfft) < 0) return "nfft must be a power of two in 64..8192";
    if (hop < 1 || hop > kSpectrumMaxHop) return "hop must be in 1..2^24";
    if (avg < 0) return "avg is negative";
    if (window) {
        if (const std::string bad = check_taps(window, nfft, "window"); !bad.empty()) return bad;
        if (std::all_of(window, window + nfft, [](float w) { return w == 0.0f; })) return "the window is all zero";
    }
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535)";
    if (max_samples < 1 || max_samples > kSpectrumMaxSamples) return "max_samples out of range (1..2^24)";
    return "";
}

SpectrumHip::SpectrumHip(int nfft, int hop, int avg, const float* window, int shifted, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = check_args(nfft, hop, avg, window, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    nfft_ = nfft; log2_ = spectrum_log2(nfft); hop_ = hop; avg_ = avg; shifted_ = shifted ? 1 : 0;
    std::vector<float> w((size_t)nfft);
    if (window) std::copy(window, window + nfft, w.begin());
    else spectrum_window(kSpectrumHann, nfft, w.data());
    const std::vector<float> staged = fft_twiddles_staged(nfft, log2_); // the table's entries in stage order (SpecArgs::tw); nfft - 1 of them
    window_power_ = spectrum_window_power(w.data(), nfft);
    // the chunk sums of the largest call, where a row of it has more than one chunk
    int seg = 0;
    spectrum_geometry(nfft, hop, avg, max_samples, &seg, nullptr, nullptr);
    const size_t row_segs = avg > 0 ? (size_t)avg : (size_t)seg, rows = avg > 0 ? (size_t)(seg / avg) : (seg > 0 ? 1 : 0);
    const size_t cpr = (row_segs + kSpectrumChunk - 1) / kSpectrumChunk;
    scratch_floats_ = cpr > 1 ? (size_t)max_streams * rows * cpr * nfft : 0;
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the window", alloc(&d_window_, (size_t)nfft));
    HIP_OK_AS("hipMalloc of the twiddles", alloc(&d_twiddles_, (size_t)nfft));
    if (scratch_floats_) HIP_OK_AS("hipMalloc of the chunk sums", alloc(&d_scratch_, scratch_floats_));
    HIP_OK(hipMemcpy(d_window_, w.data(), (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_twiddles_, staged.data(), (size_t)nfft * sizeof(float2), hipMemcpyHostToDevice));
    // 8192 points with their pads are above the 64 KiB a kernel gets unasked. The attribute belongs to the kernel, not to the handle
    HIP_OK(hipFuncSetAttribute((const void*)spectrum_kernel<13>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(13)));
}

int SpectrumHip::process_device(const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    int seg = 0, rows = 0;
    if (spectrum_geometry(nfft_, hop_, avg_, n_in, &seg, &rows, nullptr)) { call_err_.argument("n_in out of range"); return -1; }
    if (rows == 0 || n_streams <= 0) return 0; // nothing is written
    const int row_segs = avg_ > 0 ? avg_ : seg;
    const int cpr = (row_segs + kSpectrumChunk - 1) / kSpectrumChunk;
    const int64_t blocks = (int64_t)n_streams * rows * cpr;
    if (blocks > 0x7fffffff) { call_err_.argument("the call needs more than 2^31 - 1 workgroups"); return -1; }
    const bool direct = cpr == 1;
    if (!direct && (size_t)blocks * nfft_ > scratch_floats_) { call_err_.argument("the call exceeds the handle's scratch buffer"); return -1; }
    SpecArgs a;
    a.in = reinterpret_cast<const float2*>(d_in); a.in_stride = in_stride;
    a.window = d_window_; a.tw = d_twiddles_;
    a.partial = d_scratch_; a.out = d_out; a.out_stride = out_stride;
    a.hop = hop_; a.n_rows = rows; a.cpr = cpr; a.row_segs = row_segs;
    a.shift_mask = shifted_ ? nfft_ / 2 : 0;
    a.direct = direct ? 1 : 0;
    a.scale = (float)(1.0 / ((double)row_segs * window_power_));
    switch (log2_) {
    case 6: launch<6>(a, (unsigned)blocks, stream); break;
    case 7: launch<7>(a, (unsigned)blocks, stream); break;
    case 8: launch<8>(a, (unsigned)blocks, stream); break;
    case 9: launch<9>(a, (unsigned)blocks, stream); break;
    case 10: launch<10>(a, (unsigned)blocks, stream); break;
    case 11: launch<11>(a, (unsigned)blocks, stream); break;
    case 12: launch<12>(a, (unsigned)blocks, stream); break;
    default: launch<13>(a, (unsigned)blocks, stream); break;
    }
    if (launched("spectrum kernel launch")) return -1;
    if (!direct) {
        const dim3 grid((unsigned)(n_streams * rows), (unsigned)(nfft_ / kFinishThreads));
        hipLaunchKernelGGL(spectrum_finish_kernel, grid, dim3(kFinishThreads), 0, stream, d_scratch_, d_out, (long long)out_stride, nfft_, rows, cpr,
                           a.shift_mask, a.scale);
        if (launched("spectrum finish kernel launch")) return -1;
    }
    return 0;
}

} // namespace dvbs2
