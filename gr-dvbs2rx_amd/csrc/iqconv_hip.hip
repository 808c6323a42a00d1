// iqconv_hip.hip -- see iqconv_hip.h.
#include "iqconv_hip.h"
#include <cmath>
#include <cstring>
#include <type_traits>
#include "iqconv_math.hpp"

#pragma clang fp contract(off) // the arithmetic is pinned: every product and sum rounded on its own (the library is built -ffp-contract=off as well)

namespace dvbs2 {

int iqconv_bytes(int format) { return format == kIqU8 || format == kIqS8 ? 2 : format == kIqS16 ? 4 : -1; }

std::string iqconv_check(int format, float gain, int max_streams, int max_samples)
{
    if (iqconv_bytes(format) < 0) return "format is not one of DVBS2_IQ_U8, DVBS2_IQ_S8, DVBS2_IQ_S16";
    if (!std::isfinite(gain) || gain <= 0.0f) return "gain must be finite and positive";
    if (gain < kIqGainMin || gain > kIqGainMax) return "gain out of range (2^-64..2^64)";
    if (max_streams < 1 || max_streams > 65535) return "max_streams out of range (1..65535)";
    if (max_samples < 1 || max_samples > (1 << 30)) return "max_samples out of range (1..2^30)";
    return "";
}

namespace {

// the code at component j of a row that starts at any address: memcpy, so that an odd host address is no misaligned access
template <int kFmt> int host_code(const uint8_t* p, int64_t j)
{
    if constexpr (kFmt == kIqU8) return p[j];
    else if constexpr (kFmt == kIqS8) return (int8_t)p[j];
    else { int16_t c; std::memcpy(&c, p + 2 * j, 2); return c; }
}

template <int kFmt> void host_put(uint8_t* p, int64_t j, int c)
{
    if constexpr (kFmt == kIqS16) { const int16_t v = (int16_t)c; std::memcpy(p + 2 * j, &v, 2); }
    else p[j] = (uint8_t)c;
}

template <int kFmt> void unpack_host_as(float gain, const uint8_t* in, int64_t n, float* out, uint64_t* stats)
{
    const float scale = iq_unpack_scale<kFmt>(gain);
    uint64_t clipped = 0, energy = 0;
    for (int64_t j = 0; j < 2 * n; j++) {
        const int c = host_code<kFmt>(in, j), d = iq_level<kFmt>(c);
        out[j] = iq_unpack<kFmt>(c, scale);
        clipped += iq_on_rail<kFmt>(c);
        energy += (uint64_t)((int64_t)d * d);
    }
    if (stats) { stats[0] += (uint64_t)n; stats[1] += clipped; stats[2] += energy; }
}

template <int kFmt> void pack_host_as(float gain, const float* in, int64_t n, uint8_t* out, uint64_t* stats)
{
    uint64_t clipped = 0, energy = 0;
    for (int64_t j = 0; j < 2 * n; j++) {
        bool clip;
        const int c = iq_pack<kFmt>(in[j], gain, &clip), d = iq_level<kFmt>(c);
        host_put<kFmt>(out, j, c);
        clipped += clip;
        energy += (uint64_t)((int64_t)d * d);
    }
    if (stats) { stats[0] += (uint64_t)n; stats[1] += clipped; stats[2] += energy; }
}

} // namespace

void iqconv_unpack_host(int format, float gain, const void* in, int64_t n, float* out, uint64_t* stats)
{
    const uint8_t* p = static_cast<const uint8_t*>(in);
    if (format == kIqU8) unpack_host_as<kIqU8>(gain, p, n, out, stats);
    else if (format == kIqS8) unpack_host_as<kIqS8>(gain, p, n, out, stats);
    else unpack_host_as<kIqS16>(gain, p, n, out, stats);
}

void iqconv_pack_host(int format, float gain, const float* in, int64_t n, void* out, uint64_t* stats)
{
    uint8_t* p = static_cast<uint8_t*>(out);
    if (format == kIqU8) pack_host_as<kIqU8>(gain, in, n, p, stats);
    else if (format == kIqS8) pack_host_as<kIqS8>(gain, in, n, p, stats);
    else pack_host_as<kIqS16>(gain, in, n, p, stats);
}

namespace {

// native vectors: an access of 16 bytes stays one instruction
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

constexpr int kUnpackBatch = 8, kPackBatch = 4; // pieces of a lane whose loads are issued together (measured: notes/iqconv.md)
static_assert(kIqPieces % kUnpackBatch == 0 && kIqPieces % kPackBatch == 0, "a lane's pieces go in whole batches");

// component k (0..3) of the code words of a piece: one dword (u8, s8) or two (s16)
template <int kFmt> __device__ inline int code_of(const uint32_t* w, int k)
{
    if constexpr (kFmt == kIqU8) return (int)((w[0] >> (8 * k)) & 0xFFu);
    else if constexpr (kFmt == kIqS8) return (int)(int8_t)(w[0] >> (8 * k));
    else return (int)(int16_t)(w[k >> 1] >> (16 * (k & 1)));
}

template <int kFmt> __device__ inline void put_code(uint32_t* w, int k, int c)
{
    if constexpr (kFmt == kIqS16) w[k >> 1] |= ((uint32_t)c & 0xFFFFu) << (16 * (k & 1));
    else w[0] |= ((uint32_t)c & 0xFFu) << (8 * k);
}

// of one lane, at most 64 components: d * d is at most 255^2 for the 8-bit formats, whose sum fits 32 bits, and 2^30 for s16
template <int kFmt> struct IqTally {
    typename std::conditional<kFmt == kIqS16, unsigned long long, unsigned>::type energy = 0;
    unsigned clipped = 0;
};

template <int kFmt> __device__ inline void tally(IqTally<kFmt>& t, int c, bool clipped)
{
    const int d = iq_level<kFmt>(c);
    t.energy += (unsigned)(d * d);
    t.clipped += clipped;
}

// lanes -> wave -> workgroup -> one atomicAdd per counter that has something to add. Every lane of the workgroup calls it. The row's
// first workgroup adds the row's samples: atomics on one row's counters cost their time in full (notes/iqconv.md), so none is spent on
// what is known beforehand.
template <int kFmt> __device__ inline void tally_flush(const IqTally<kFmt>& t, long long n2, unsigned long long* row_stats)
{
    __shared__ unsigned long long s_energy[kIqLanes / 64];
    __shared__ unsigned s_clipped[kIqLanes / 64];
    unsigned long long e = t.energy;
    unsigned c = t.clipped;
    for (int off = 32; off; off >>= 1) { e += __shfl_down(e, off); c += __shfl_down(c, off); }
    if ((threadIdx.x & 63) == 0) { s_energy[threadIdx.x >> 6] = e; s_clipped[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kIqLanes / 64; w++) { e += s_energy[w]; c += s_clipped[w]; }
        if (blockIdx.x == 0) atomicAdd(&row_stats[0], (unsigned long long)(n2 / 2));
        if (c) atomicAdd(&row_stats[1], (unsigned long long)c);
        if (e) atomicAdd(&row_stats[2], e);
    }
}

// A piece at a row's end: the samples of components j0 and j0 + 2 (j0 is even) that lie inside the row, byte or short loads.
template <int kFmt, bool kStats> __device__ inline void unpack_edge(const uint8_t* src, float* dst, long long j0, long long n2, float scale, IqTally<kFmt>& t)
{
    for (int s = 0; s < 2; s++) {
        const long long j = j0 + 2 * s;
        if (j < 0 || j >= n2) continue;
        int c[2];
        for (int k = 0; k < 2; k++) {
            if constexpr (kFmt == kIqU8) c[k] = src[j + k];
            else if constexpr (kFmt == kIqS8) c[k] = (int8_t)src[j + k];
            else c[k] = reinterpret_cast<const int16_t*>(src)[j + k];
            if (kStats) tally<kFmt>(t, c[k], iq_on_rail<kFmt>(c[k]));
        }
        *reinterpret_cast<v2f*>(dst + j) = v2f{ iq_unpack<kFmt>(c[0], scale), iq_unpack<kFmt>(c[1], scale) };
    }
}

// Workgroup (x, y): pieces [P x, P x + P) of row y, P = kIqLanes * kIqPieces. Piece p holds the components 4 p - h .. 4 p - h + 3 of the row, h (0 or 2)
// such that its floats are 16-byte aligned; its codes start `shift` bytes into an aligned dword. kWide: h == 0 and shift == 0 in
// every row, and the codes of a piece are aligned to their size.
template <int kFmt, bool kWide, bool kStats>
__global__ __launch_bounds__(kIqLanes) void iq_unpack_kernel(const uint8_t* in, long long in_stride, float* out, long long out_stride, float scale,
                                                             long long n2, unsigned long long* stats)
{
    constexpr int W = IqFormat<kFmt>::bytes, cs = IqFormat<kFmt>::bytes; // code dwords of a piece, bytes of a code
    const int row = blockIdx.y;
    const uint8_t* src = in + (long long)row * in_stride * (2 * cs);
    float* dst = out + (long long)row * out_stride * 2;
    const int h = kWide ? 0 : (int)(((uintptr_t)dst >> 3) & 1) * 2;
    const uintptr_t c_lo = (uintptr_t)src, c_hi = c_lo + (uintptr_t)(n2 * cs);
    const int shift = kWide ? 0 : (int)((c_lo - (uintptr_t)(h * cs)) & 3);
    const long long p0 = (long long)blockIdx.x * (kIqLanes * kIqPieces) + threadIdx.x;
    IqTally<kFmt> t;
    for (int batch = 0; batch < kIqPieces / kUnpackBatch; batch++) {
        uint32_t w[kUnpackBatch][W];
        long long j0[kUnpackBatch];
        bool whole[kUnpackBatch];
#pragma unroll
        for (int k = 0; k < kUnpackBatch; k++) {
            j0[k] = 4 * (p0 + (long long)(batch * kUnpackBatch + k) * kIqLanes) - h;
            const uintptr_t a = c_lo + (uintptr_t)(j0[k] * cs);
            if (kWide) {
                whole[k] = j0[k] + 4 <= n2;
                if (whole[k]) {
                    if constexpr (W == 1) w[k][0] = *reinterpret_cast<const uint32_t*>(a);
                    else { const v2u v = *reinterpret_cast<const v2u*>(a); w[k][0] = v.x; w[k][1] = v.y; }
                }
            } else {
                // the aligned dwords that hold the piece's codes: W of them, one more when the codes start inside a dword
                const uintptr_t a_al = a - (uintptr_t)shift;
                whole[k] = j0[k] >= 0 && a_al >= c_lo && a_al + 4u * (W + (shift != 0)) <= c_hi;
                if (whole[k]) {
                    uint32_t d[W + 1];
                    for (int i = 0; i < W; i++) d[i] = reinterpret_cast<const uint32_t*>(a_al)[i];
                    d[W] = shift ? reinterpret_cast<const uint32_t*>(a_al)[W] : 0u;
                    for (int i = 0; i < W; i++) w[k][i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> (8 * shift));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kUnpackBatch; k++) {
            if (whole[k]) {
                v4f y;
                for (int i = 0; i < 4; i++) {
                    const int c = code_of<kFmt>(w[k], i);
                    y[i] = iq_unpack<kFmt>(c, scale);
                    if (kStats) tally<kFmt>(t, c, iq_on_rail<kFmt>(c));
                }
                *reinterpret_cast<v4f*>(dst + j0[k]) = y;
            } else unpack_edge<kFmt, kStats>(src, dst, j0[k], n2, scale, t);
        }
    }
    if (kStats) tally_flush(t, n2, stats + 3 * row);
}

// A piece at a row's end: its components inside the row one by one, byte or short stores.
template <int kFmt, bool kStats> __device__ inline void pack_edge(const float* src, uint8_t* dst, long long j0, long long n2, float gain, IqTally<kFmt>& t)
{
    for (int k = 0; k < 4; k++) {
        const long long j = j0 + k;
        if (j < 0 || j >= n2) continue;
        bool clipped;
        const int c = iq_pack<kFmt>(src[j], gain, &clipped);
        if constexpr (kFmt == kIqS16) reinterpret_cast<int16_t*>(dst)[j] = (int16_t)c;
        else dst[j] = (uint8_t)c;
        if (kStats) tally<kFmt>(t, c, clipped);
    }
}

// Workgroup (x, y): pieces [P x, P x + P) of row y, P = kIqLanes * kIqPieces. Piece p holds the components 4 p - h .. 4 p - h + 3 of the row, h (0..3) such
// that its codes are aligned to their size (4 or 8 bytes); its floats are 8-byte aligned when h is even, else 4-byte. kWide: h == 0 and
// the floats of a piece are 16-byte aligned, in every row.
template <int kFmt, bool kWide, bool kStats>
__global__ __launch_bounds__(kIqLanes) void iq_pack_kernel(const float* in, long long in_stride, uint8_t* out, long long out_stride, float gain,
                                                           long long n2, unsigned long long* stats)
{
    constexpr int W = IqFormat<kFmt>::bytes, cs = IqFormat<kFmt>::bytes;
    const int row = blockIdx.y;
    const float* src = in + (long long)row * in_stride * 2;
    uint8_t* dst = out + (long long)row * out_stride * (2 * cs);
    const int h = kWide ? 0 : (int)(((uintptr_t)dst & (4 * cs - 1)) / cs);
    const long long p0 = (long long)blockIdx.x * (kIqLanes * kIqPieces) + threadIdx.x;
    IqTally<kFmt> t;
    for (int batch = 0; batch < kIqPieces / kPackBatch; batch++) {
        v4f x[kPackBatch];
        long long j0[kPackBatch];
        bool whole[kPackBatch];
#pragma unroll
        for (int k = 0; k < kPackBatch; k++) {
            j0[k] = 4 * (p0 + (long long)(batch * kPackBatch + k) * kIqLanes) - h;
            whole[k] = j0[k] >= 0 && j0[k] + 4 <= n2;
            if (!whole[k]) continue;
            const float* s = src + j0[k];
            if (kWide) x[k] = *reinterpret_cast<const v4f*>(s);
            else if ((h & 1) == 0) {
                x[k].xy = reinterpret_cast<const v2f*>(s)[0];
                x[k].zw = reinterpret_cast<const v2f*>(s)[1];
            } else x[k] = v4f{ s[0], s[1], s[2], s[3] };
        }
#pragma unroll
        for (int k = 0; k < kPackBatch; k++) {
            if (whole[k]) {
                uint32_t w[W] = {};
                for (int i = 0; i < 4; i++) {
                    bool clipped;
                    const int c = iq_pack<kFmt>(x[k][i], gain, &clipped);
                    put_code<kFmt>(w, i, c);
                    if (kStats) tally<kFmt>(t, c, clipped);
                }
                uint8_t* d = dst + j0[k] * cs;
                if constexpr (W == 1) *reinterpret_cast<uint32_t*>(d) = w[0];
                else *reinterpret_cast<v2u*>(d) = v2u{ w[0], w[1] };
            } else pack_edge<kFmt, kStats>(src, dst, j0[k], n2, gain, t);
        }
    }
    if (kStats) tally_flush(t, n2, stats + 3 * row);
}

#define IQ_PICK_OF(kernel, fmt, wide, stats) \
    ((wide) ? ((stats) ? kernel<fmt, true, true> : kernel<fmt, true, false>) : ((stats) ? kernel<fmt, false, true> : kernel<fmt, false, false>))
#define IQ_PICK(kernel, format, wide, stats) \
    ((format) == kIqU8 ? IQ_PICK_OF(kernel, kIqU8, wide, stats) : (format) == kIqS8 ? IQ_PICK_OF(kernel, kIqS8, wide, stats) : IQ_PICK_OF(kernel, kIqS16, wide, stats))

// the wide path: floats 16-byte aligned and codes aligned to a piece's (4 bytes, s16: 8), in every row
bool wide_rows(int format, const void* codes, int64_t code_stride, const float* floats, int64_t float_stride, int n_streams)
{
    const uintptr_t piece = 2 * (uintptr_t)iqconv_bytes(format);
    return (uintptr_t)floats % 16 == 0 && (uintptr_t)codes % piece == 0 && (n_streams == 1 || ((code_stride | float_stride) & 1) == 0);
}

dim3 grid_of(int n_samples, int n_streams, bool wide)
{
    const long long pieces = (2LL * n_samples + (wide ? 0 : 3) + 3) / 4; // an edge row starts up to 3 components into its first piece
    return dim3((unsigned)((pieces + kIqLanes * kIqPieces - 1) / (kIqLanes * kIqPieces)), (unsigned)n_streams);
}

} // namespace

IqconvHip::IqconvHip(int format, float gain, int max_streams, int max_samples, int device)
    : StreamStage(max_streams, max_samples, device)
{
    if (const std::string bad = iqconv_check(format, gain, max_streams, max_samples); !bad.empty()) { err_.argument(bad); return; }
    format_ = format;
    gain_ = gain;
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
}

int IqconvHip::set_gain(float gain)
{
    call_err_ = {};
    if (const std::string bad = iqconv_check(format_, gain, 1, 1); !bad.empty()) { call_err_.argument(bad); return -1; }
    gain_ = gain;
    return 0;
}

int IqconvHip::unpack_device(const void* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out, int64_t out_stride, uint64_t* d_stats,
                             hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_samples == 0 || n_streams == 0) return 0;
    const bool wide = wide_rows(format_, d_in, in_stride, d_out, out_stride, n_streams);
    const float scale = format_ == kIqS16 ? iq_unpack_scale<kIqS16>(gain_) : iq_unpack_scale<kIqU8>(gain_);
    auto kernel = IQ_PICK(iq_unpack_kernel, format_, wide, d_stats != nullptr);
    hipLaunchKernelGGL(kernel, grid_of(n_samples, n_streams, wide), dim3(kIqLanes), 0, stream, static_cast<const uint8_t*>(d_in), (long long)in_stride,
                       d_out, (long long)out_stride, scale, 2LL * n_samples, reinterpret_cast<unsigned long long*>(d_stats));
    return launched("iqconv unpack kernel launch");
}

int IqconvHip::pack_device(const float* d_in, int64_t in_stride, int n_samples, int n_streams, void* d_out, int64_t out_stride, uint64_t* d_stats,
                           hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_samples == 0 || n_streams == 0) return 0;
    const bool wide = wide_rows(format_, d_out, out_stride, d_in, in_stride, n_streams);
    auto kernel = IQ_PICK(iq_pack_kernel, format_, wide, d_stats != nullptr);
    hipLaunchKernelGGL(kernel, grid_of(n_samples, n_streams, wide), dim3(kIqLanes), 0, stream, d_in, (long long)in_stride, static_cast<uint8_t*>(d_out),
                       (long long)out_stride, gain_, 2LL * n_samples, reinterpret_cast<unsigned long long*>(d_stats));
    return launched("iqconv pack kernel launch");
}

} // namespace dvbs2
