// symsync_hip.hip -- see symsync_hip.h.
#include "symsync_hip.h"
#include "rrc_pulse.h"
#include <cmath>
#include <cstring>
#include <new>

namespace dvbs2 {

void symsync_loop_constants(int sps, float loop_bw, float damping, float rolloff, float* Kp, float* K1, float* K2)
{
    // Detector gain: the slope at the origin of the Gardner S-curve for unit symbol energy and unit channel gain (Rice, "Digital
    // Communications", eq. 8.47), taken as rise over run across 2/1000 of a symbol. Then the proportional and integral gains of
    // the second-order loop for a noise bandwidth given per symbol (eq. C.56, C.60), divided by the detector gain and by the
    // counter's gain of -1 (it counts down). The values are those of lib/symbol_sync_cc_impl.cc:156-199: every quantity is
    // rounded to float once, and sub-expressions are double exactly where a double operand makes them so there.
    const float grid = 1e3;
    const float curve_scale = (float)(sin(M_PI * (double)rolloff / 2) / (4 * M_PI * (double)(1 - (rolloff * rolloff / 4))));
    const float run = (float)(2.0 / (double)grid);
    const float rise = (float)((double)(8 * curve_scale) * sin(2 * M_PI / (double)grid));
    const float detector_gain = rise / run;
    const float bw_per_sample = loop_bw / (float)sps;
    const float theta = (float)((double)bw_per_sample / ((double)damping + 1.0 / (double)(4 * damping)));
    const float denom = 1 + 2 * damping * theta + theta * theta;
    const float prop = (4 * damping * theta) / denom;
    const float integ = (4 * (theta * theta)) / denom;
    const float counter_gain = -1;
    if (Kp) *Kp = detector_gain;
    if (K1) *K1 = prop / (detector_gain * counter_gain);
    if (K2) *K2 = integ / (detector_gain * counter_gain);
}

int symsync_geometry(int sps, int rrc_delay, int n_subfilt, int interp, int* subfilt_len, int* subfilt_delay, int* history)
{
    if (sps < 2 || (sps & 1) || sps > 64 || rrc_delay < 1 || rrc_delay > 64 || n_subfilt < 2 || n_subfilt > 4096 || interp < 0 || interp > 3)
        return -1;
    // ceil((2 n_subfilt sps rrc_delay + 1) / n_subfilt) of :68-71 in integers (the reference's float form loses the + 1 beyond 2^24)
    const int L = 2 * sps * rrc_delay + 1;
    if (subfilt_len) *subfilt_len = L;
    if (subfilt_delay) *subfilt_delay = (L - 1) / 2;
    if (history) *history = (interp == 0 ? L - 1 : interp == 1 ? 1 : 3) + sps / 2;
    return 0;
}

int symsync_taps(int sps, float rolloff, int rrc_delay, int n_subfilt, float* bank)
{
    int L;
    if (!bank || symsync_geometry(sps, rrc_delay, n_subfilt, 0, &L, nullptr, nullptr) || !(rolloff >= 0.0f && rolloff <= 1.0f)) return -1;
    const int poly_sps = n_subfilt * sps, n = 2 * poly_sps * rrc_delay + 1; // :83-84
    std::vector<double> h((size_t)n_subfilt * L, 0.0);                         // zero padded to a multiple of n_subfilt (:90-91)
    double sum = 0.0;
    for (int i = 0; i < n; i++) { h[i] = rrc((double)(i - (n - 1) / 2) / poly_sps, (double)rolloff); sum += h[i]; }
    // the taps sum to the gain, n_subfilt (firdes's convention); subfilter i = taps i + j n_subfilt, flipped (:98-110)
    for (int i = 0; i < n_subfilt; i++)
        for (int j = 0; j < L; j++) bank[(size_t)i * L + (L - 1 - j)] = (float)(h[i + (size_t)j * n_subfilt] * n_subfilt / sum);
    return 0;
}

namespace {

struct SymSyncIo {
    const float2* in; long long in_stride; const int* n_in;
    float2* out; long long out_stride; int max_out;
    long long* strobe; double* mu;
};

constexpr int kMask = kSymsyncRing - 1;
constexpr int kPer = kSymsyncChunk / 64;

__device__ inline float2 cmul(float2 a, float c) { return make_float2(a.x * c, a.y * c); }  // complex * float
__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

// one coefficient row of a Farrow structure over the four-sample window, summed from zero in window order
__device__ inline float2 farrow_row(const float2 (&w)[4], const float (&c)[4])
{
    float2 acc = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 4; i++) acc = cadd(acc, cmul(w[i], c[i]));
    return acc;
}

// the interpolant at basepoint b with fractional offset mu; ring holds the samples b - (what the method reads) .. b + 1
template <int INTERP>
__device__ inline float2 interpolate(const float2* __restrict__ ring, const float* __restrict__ sb, const SymSyncGeom& g, int b, double mu, int j)
{
    if (INTERP == 0) {
        const double p = floor((double)g.n_subfilt * mu); // :125
        const int idx = p >= 0.0 ? (p < (double)g.n_subfilt ? (int)p : g.n_subfilt - 1) : 0;
        const float* __restrict__ f = sb + idx * g.subfilt_len;
        const int start = b + 2 - g.subfilt_len; // :130
        float ar = 0.0f, ai = 0.0f;
        for (int t = j; t < g.subfilt_len; t += 32) {
            const float2 x = ring[(start + t) & kMask];
            const float c = f[t];
            ar += x.x * c; ai += x.y * c;
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) { ar += __shfl_xor(ar, m); ai += __shfl_xor(ai, m); }
        return make_float2(ar, ai);
    }
    // Farrow forms (Rice, eq. 8.61, 8.76-8.78, tables 8.4.1 / 8.4.2): a polynomial in mu whose coefficients are fixed
    // combinations of the window w = x[b + 1], x[b], x[b - 1], x[b - 2]; each row is summed from zero in window order and the
    // polynomial is nested from the highest power down, which is the order of lib/symbol_sync_cc_impl.cc:23-66
    const float m = (float)mu;
    float2 w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = ring[(b + 1 - i) & kMask];
    if (INTERP == 1) return cadd(cmul(w[0], m), cmul(w[1], 1 - m));
    const float sixth = (float)(1.0 / 6), third = (float)(1.0 / 3);
    if (INTERP == 2) {
        const float sq[4] = { .5f, -.5f, -.5f, .5f }, lin[4] = { -.5f, 1.5f, -.5f, -.5f };
        return cadd(cmul(cadd(cmul(farrow_row(w, sq), m), farrow_row(w, lin)), m), w[2]);
    }
    const float cu[4] = { sixth, -.5f, .5f, -sixth }, sq[4] = { 0.0f, .5f, -1.0f, .5f }, lin[4] = { -sixth, 1.0f, -.5f, -third };
    return cadd(cmul(cadd(cmul(cadd(cmul(farrow_row(w, cu), m), farrow_row(w, sq)), m), farrow_row(w, lin)), m), w[2]);
}

// one wavefront per stream. The input of a call is the virtual buffer V: V[0 .. H) the history, V[H .. H + n_in) the samples
template <int INTERP>
__global__ __launch_bounds__(64) void symsync_kernel(SymSyncIo io, SymSyncGeom g, const float* __restrict__ bank, float2* __restrict__ hist,
                                                     SymSyncState* __restrict__ st, SymSyncResult* __restrict__ res)
{
    extern __shared__ float2 lds[];
    float2* ring = lds;
    float* sb = reinterpret_cast<float*>(lds + kSymsyncRing);
    const int s = blockIdx.x, l = threadIdx.x, H = g.history;
    SymSyncState S = st[s];
    const int n_in = io.n_in[s];
    if (S.status || (!S.init && n_in < 2)) { // uniform: the whole wavefront leaves
        if (l == 0) { SymSyncResult r = { 0, 0, S.status, 0 }; res[s] = r; }
        return;
    }
    const int total = H + n_in;
    const float2* __restrict__ x = io.in + (long long)s * io.in_stride;
    const float2* __restrict__ hin = hist + ((size_t)s * 2 + S.parity) * H;
    float2* __restrict__ hout = hist + ((size_t)s * 2 + (S.parity ^ 1)) * H;
    auto fetch = [&](int i) {
        float2 v = make_float2(0.0f, 0.0f);
        if (i < H) v = hin[i];
        else if (i < total) v = x[i - H];
        return v;
    };
    if (INTERP == 0)
        for (int i = l; i < g.n_subfilt * g.subfilt_len; i += 64) sb[i] = bank[i];

    int loaded = 0; // the ring holds V[loaded - kSymsyncRing .. loaded), pf holds V[loaded .. loaded + kSymsyncChunk)
    float2 pf[kPer];
#pragma unroll
    for (int c = 0; c < kPer; c++) pf[c] = fetch(c * 64 + l);
    // a strobe at n reads V[n - H .. n] and H <= kSymsyncRing - kSymsyncChunk, so a chunk stored when n >= loaded overwrites
    // nothing a strobe at or after n reads
    auto reach = [&](int n) {
        while (n >= loaded) {
            __syncthreads();
#pragma unroll
            for (int c = 0; c < kPer; c++) ring[(loaded + c * 64 + l) & kMask] = pf[c];
            loaded += kSymsyncChunk;
#pragma unroll
            for (int c = 0; c < kPer; c++) pf[c] = fetch(loaded + c * 64 + l); // in flight while the ring is walked
            __syncthreads();
        }
    };
    __syncthreads();

    int n = H - 1, k = 0, status = 0;
    if (!S.init) { // :314-325
        reach(H);
        S.last_xi = ring[H & kMask];
        S.init = 1;
        n += 2;
    }
    const int mid = g.sps / 2, half = l >> 5, j = l & 31;
    const double step = 1.0 / (double)(float)g.sps; // d_nominal_step
    float2* __restrict__ out = io.out + (long long)s * io.out_stride;
    while ((long long)n + S.jump < total && k < io.max_out) {
        n += S.jump;
        reach(n);
        const int m_k = n - 1;
        const float2 v = interpolate<INTERP>(ring, sb, g, m_k - (half ? mid : 0), S.mu, j);
        const float2 o = make_float2(__shfl(v.x, 0), __shfl(v.y, 0)), zc = make_float2(__shfl(v.x, 32), __shfl(v.y, 32));
        if (l == 0) {
            out[k] = o;
            if (io.strobe) io.strobe[(long long)s * io.out_stride + k] = S.n_read + m_k - H;
            if (io.mu) io.mu[(long long)s * io.out_stride + k] = S.mu;
        }
        const float e = zc.x * (S.last_xi.x - o.x) + zc.y * (S.last_xi.y - o.y); // :347-348
        S.last_xi = o;
        k++;
        const double vp = (double)(g.K1 * e); // :352-363
        S.vi += (double)(g.K2 * e);
        const double pi_out = vp + S.vi;
        const double W1 = step + pi_out, W2 = step + S.vi;
        if (W1 != W1 || W2 != W2) { status = 2; break; }
        if (!(W1 > 0.0 && W2 > 0.0)) { status = 1; break; }
        const double jd = floor((S.cnt - W1) / W2) + 2.0; // :372
        if (!(jd >= 1.0 && jd <= (double)kSymsyncMaxJump)) { status = 3; break; }
        S.jump = (int)jd;
        if (S.jump > 1) { // :375-390
            const double cnt_basepoint = S.cnt - W1 - ((S.jump - 2) * W2);
            S.mu = cnt_basepoint / W2;
            S.cnt = cnt_basepoint - W2 + 1;
        } else {
            S.mu = S.cnt / W1;
            S.cnt = S.cnt - W1 + 1;
        }
    }
    const int consumed = n + 1 - H; // :441
    if (consumed > 0) { // the H samples before the first unconsumed one, into the other buffer
        for (int i = l; i < H; i += 64) hout[i] = fetch(consumed + i);
        S.parity ^= 1;
    }
    if (l == 0) {
        S.n_read += consumed;
        S.status = status;
        st[s] = S;
        SymSyncResult r = { k, consumed, status, 0 };
        res[s] = r;
    }
}

} // namespace

std::string SymSyncHip::check_args(int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp, int max_streams,
                                   int max_samples)
{
    int L, D, H;
    if (symsync_geometry(sps, rrc_delay, n_subfilt, interp, &L, &D, &H))
        return "sps must be an even integer in 2..64, rrc_delay in 1..64, n_subfilt in 2..4096, interp_method in 0..3";
    if (!(rolloff >= 0.0f && rolloff <= 1.0f) || !(loop_bw >= 0.0f) || !(damping >= 0.0f) || loop_bw - loop_bw != 0.0f || damping - damping != 0.0f)
        return "rolloff must lie in [0, 1], loop_bw and damping must be finite and not negative";
    if (max_streams < 1 || max_streams > (1 << 16)) return "max_streams out of range (1..65536)";
    if (max_samples < 2 || max_samples > (1 << 30)) return "max_samples out of range (2..2^30)";
    if (interp == 0 && kSymsyncRing * sizeof(float2) + (size_t)n_subfilt * L * sizeof(float) > (size_t)kSymsyncMaxLds)
        return "the subfilter bank does not fit the LDS";
    if (H > kSymsyncRing - kSymsyncChunk) return "the history does not fit the LDS ring";
    return "";
}

SymSyncHip::SymSyncHip(int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp, const float* bank,
                       int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = check_args(sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    int L, D, H;
    symsync_geometry(sps, rrc_delay, n_subfilt, interp, &L, &D, &H);
    const size_t bank_bytes = (size_t)n_subfilt * L * sizeof(float);
    g_.sps = sps; g_.interp = interp; g_.n_subfilt = n_subfilt; g_.subfilt_len = L; g_.subfilt_delay = D; g_.history = H;
    symsync_loop_constants(sps, loop_bw, damping, rolloff, &Kp_, &g_.K1, &g_.K2);
    std::vector<float> taps((size_t)n_subfilt * L);
    if (bank) memcpy(taps.data(), bank, bank_bytes);
    else symsync_taps(sps, rolloff, rrc_delay, n_subfilt, taps.data());
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok || alloc(&d_bank_, taps.size()) != hipSuccess || alloc_zeroed(&d_hist_, (size_t)max_streams_ * 2 * H) != hipSuccess ||
        alloc(&d_state_, max_streams_) != hipSuccess || alloc_zeroed(&d_res_, max_streams_) != hipSuccess || alloc(&d_nin_, max_streams_) != hipSuccess ||
        hipMemcpy(d_bank_, taps.data(), bank_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        err_.argument("device setup failed"); return; // (device failure, kArgument: notes/stage_error_codes.md)
    }
    res_.resize(max_streams_);
    if (reset()) { err_.argument(call_err_.text); call_err_ = {}; } // (device failure, kArgument: notes/stage_error_codes.md)
}

int SymSyncHip::reset()
{
    Entry on(*this);
    SymSyncState s0;
    memset(&s0, 0, sizeof(s0));
    s0.cnt = 1.0 - 1.0 / (double)(float)g_.sps; // :219-225: vi 0, mu 0, jump sps, not initialised, last_xi 0
    s0.jump = g_.sps;
    std::vector<SymSyncState> all(max_streams_, s0);
    if (!on.ok || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(d_state_, all.data(), all.size() * sizeof(SymSyncState), hipMemcpyHostToDevice) != hipSuccess ||
        zero(d_hist_) != hipSuccess || zero(d_res_) != hipSuccess) { // the history starts as zeros
        call_err_.device("reset of the device state failed"); return -1;
    }
    last_streams_ = 0;
    return 0;
}

int SymSyncHip::work_device(const float2* d_in, int64_t in_stride, const int* n_in, int n_streams, float2* d_out, int64_t out_stride, int max_out,
                            int64_t* d_strobe_idx, double* d_mu, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (hipMemcpyAsync(d_nin_, n_in, (size_t)n_streams * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) {
        call_err_.device("copy of the sample counts failed"); return -1;
    }
    SymSyncIo io = { d_in, (long long)in_stride, d_nin_, d_out, (long long)out_stride, max_out, reinterpret_cast<long long*>(d_strobe_idx), d_mu };
    const size_t lds = kSymsyncRing * sizeof(float2) + (g_.interp == 0 ? (size_t)g_.n_subfilt * g_.subfilt_len * sizeof(float) : 0);
    const dim3 grid(n_streams), block(64);
    switch (g_.interp) {
    case 0: hipLaunchKernelGGL(symsync_kernel<0>, grid, block, lds, stream, io, g_, d_bank_, d_hist_, d_state_, d_res_); break;
    case 1: hipLaunchKernelGGL(symsync_kernel<1>, grid, block, lds, stream, io, g_, d_bank_, d_hist_, d_state_, d_res_); break;
    case 2: hipLaunchKernelGGL(symsync_kernel<2>, grid, block, lds, stream, io, g_, d_bank_, d_hist_, d_state_, d_res_); break;
    default: hipLaunchKernelGGL(symsync_kernel<3>, grid, block, lds, stream, io, g_, d_bank_, d_hist_, d_state_, d_res_); break;
    }
    if (launched("symsync kernel launch")) return -1;
    last_streams_ = n_streams; last_stream_ = stream;
    return 0;
}

int SymSyncHip::finish(int* n_out, int* consumed, int* status)
{
    Entry on(*this);
    if (!on.ok || hipStreamSynchronize(last_stream_) != hipSuccess ||
        (last_streams_ && hipMemcpy(res_.data(), d_res_, (size_t)last_streams_ * sizeof(SymSyncResult), hipMemcpyDeviceToHost) != hipSuccess)) {
        call_err_.device("reading the results failed"); return -1;
    }
    for (int s = 0; s < last_streams_; s++) {
        if (n_out) n_out[s] = res_[s].n_out;
        if (consumed) consumed[s] = res_[s].consumed;
        if (status) status[s] = res_[s].status;
    }
    return last_streams_;
}

int SymSyncHip::state(int s, SymSyncState* out)
{
    Entry on(*this);
    if (!on.ok || hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d_state_ + s, sizeof(SymSyncState), hipMemcpyDeviceToHost) != hipSuccess) {
        call_err_.device("reading the state failed"); return -1;
    }
    return 0;
}

} // namespace dvbs2
