// plframer_hip.hip -- see plframer_hip.h. One streaming kernel, HBM bound: 8 B in + 8 B out per data symbol, writes only for headers,
// pilots and dummy payloads. No LDS, no atomics: a thread owns one symbol PAIR and nothing is shared.
#include "plframer_hip.h"
#include <algorithm>

namespace dvbs2 {

namespace {

constexpr uint32_t kPilotBits = 0x3f3504f3u; // 0.70710678118654752440f, the (S, S) of a pilot and of a dummy frame's payload
constexpr int kMaxPayload = 360 * 90 + 22 * 36;

// (a, b) times j^rn as bit patterns: a swap and a sign flip, no arithmetic -- 0.0 becomes -0.0, a denormal stays one
// rn 0: (a, b)   1: (-b, a)   2: (-a, -b)   3: (b, -a)
__device__ inline uint2 pl_scramble(uint2 v, uint32_t rn)
{
    const bool swap = rn & 1;
    const uint32_t re = swap ? v.y : v.x, im = swap ? v.x : v.y;
    return make_uint2(re ^ (((rn ^ (rn >> 1)) & 1) << 31), im ^ ((rn >> 1) << 31));
}

// Thread (blockIdx.x, threadIdx.x) of row blockIdx.y owns symbols 2 p and 2 p + 1 of frame blockIdx.y's PLFRAME; the last row is 90 symbols
// longer when closing_plsc >= 0: the closing header lies right behind the last frame. No pair straddles a header, data or pilot boundary
// and every offset is even, so with both bases 16-byte aligned (kWide) a pair is one 16-byte load and one 16-byte store; otherwise two of 8.
template <bool kWide>
__global__ __launch_bounds__(256) void pl_framer_kernel(const uint2* __restrict__ in, const uint8_t* __restrict__ rn,
                                                        const uint4* __restrict__ hdr, const PlFramerRec* __restrict__ rec,
                                                        uint2* __restrict__ out, int closing_plsc)
{
    const PlFramerRec r = rec[blockIdx.y];
    const int s = 2 * (blockIdx.x * 256 + threadIdx.x); // first symbol of the pair, counted from the frame's start
    const int plframe_len = pl_frame_len(r.n_slots, r.n_pilots);
    const bool closing = closing_plsc >= 0 && blockIdx.y == gridDim.y - 1 && s >= plframe_len;
    if (s >= plframe_len + (closing ? 90 : 0)) return; // the spare blocks of a frame shorter than the longest one leave here
    const int n_pilots = r.n_pilots;

    uint4 v;
    if (closing) v = hdr[closing_plsc * 45 + ((s - plframe_len) >> 1)];
    else if (s < 90) v = hdr[r.plsc * 45 + (s >> 1)]; // PLHEADER: copied, not PL-scrambled
    else {
        const int k = s - 90; // index in the payload; Rn restarts with every frame
        const int blk = k / 1476;
        const bool pilot = n_pilots > 0 && k - blk * 1476 >= 1440 && blk < n_pilots;
        if (pilot || r.dummy) v = make_uint4(kPilotBits, kPilotBits, kPilotBits, kPilotBits);
        else {
            const uint2* __restrict__ x = in + r.in_offset + (k - (n_pilots > 0 ? 36 * blk : 0));
            if (kWide) v = *reinterpret_cast<const uint4*>(x);
            else { const uint2 a = x[0], b = x[1]; v = make_uint4(a.x, a.y, b.x, b.y); }
        }
        const uint32_t r2 = *reinterpret_cast<const uint16_t*>(rn + k); // Rn(k) | Rn(k + 1) << 8; k is even
        const uint2 a = pl_scramble(make_uint2(v.x, v.y), r2 & 3), b = pl_scramble(make_uint2(v.z, v.w), r2 >> 8);
        v = make_uint4(a.x, a.y, b.x, b.y);
    }
    uint2* __restrict__ y = out + r.out_offset + s;
    if (kWide) *reinterpret_cast<uint4*>(y) = v;
    else { y[0] = make_uint2(v.x, v.y); y[1] = make_uint2(v.z, v.w); }
}

} // namespace

PlFramerHip::PlFramerHip(int gold_code, int max_frames, int device) : DeviceStage(device), max_frames_(max_frames)
{
    if (gold_code < 0 || gold_code >= (1 << 18) - 1) { err_.argument("gold code out of range"); return; }
    if (max_frames_ < 1 || max_frames_ > 65535) { err_.argument("max_frames must be in 1..65535 (frames are one launch dimension)"); return; }
    std::vector<uint8_t> rn(kMaxPayload);
    pl_scrambling_rn(gold_code, rn.data(), kMaxPayload);
    std::vector<float> hdr(128 * 180);
    for (int p = 0; p < 128; p++) plheader_symbols(p, &hdr[(size_t)p * 180]);
    DeviceGuard dev_guard(device_); // the caller's current device is restored on return
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the Rn table", alloc(&d_rn_, rn.size()));
    HIP_OK_AS("hipMalloc of the PLHEADER table", alloc(&d_hdr_, hdr.size()));
    HIP_OK_AS("hipMalloc of the frame records", alloc(&d_rec_, (size_t)max_frames_));
    HIP_OK(hipMemcpy(d_rn_, rn.data(), rn.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_hdr_, hdr.data(), hdr.size() * sizeof(float), hipMemcpyHostToDevice));
}

int PlFramerHip::set_sequence(const uint8_t* plsc, int n_frames)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_ = { kSize, "n_frames exceeds max_frames" }; return -1; }
    std::vector<PlFramerRec> rec(n_frames);
    int64_t in = 0, out = 0;
    std::string why;
    if (!plframer_layout(plsc, n_frames, rec.data(), &in, &out, &why)) { call_err_.argument(why); return -1; }
    if (n_frames) HIP_RET(hipMemcpy(d_rec_, rec.data(), rec.size() * sizeof(PlFramerRec), hipMemcpyHostToDevice));
    rec_.swap(rec); in_syms_ = in; out_syms_ = out;
    longest_.resize(n_frames);
    for (int f = 0, m = 0; f < n_frames; f++) longest_[f] = m = std::max(m, pl_frame_len(rec_[f].n_slots, rec_[f].n_pilots));
    return 0;
}

int PlFramerHip::frame_device(const float* d_xfecframes, int n_frames, int closing_plsc, float* d_plframes, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > this->n_frames()) { call_err_ = { kSize, "n_frames exceeds the sequence" }; return -1; }
    if (n_frames == 0) return 0;
    if (closing_plsc >= 0 && plframer_refusal(closing_plsc)) { call_err_.argument(std::string("closing_plsc ") + plframer_refusal(closing_plsc)); return -1; }
    if (((uintptr_t)d_xfecframes | (uintptr_t)d_plframes) & 7) { call_err_.argument("symbol buffers must be 8-byte aligned"); return -1; }
    const bool wide = (((uintptr_t)d_xfecframes | (uintptr_t)d_plframes) & 15) == 0;
    const PlFramerRec& last = rec_[n_frames - 1];
    const int longest = std::max(longest_[n_frames - 1], pl_frame_len(last.n_slots, last.n_pilots) + (closing_plsc >= 0 ? 90 : 0));
    const dim3 grid((longest / 2 + 255) / 256, n_frames);
    hipLaunchKernelGGL(wide ? pl_framer_kernel<true> : pl_framer_kernel<false>, grid, dim3(256), 0, stream,
                       reinterpret_cast<const uint2*>(d_xfecframes), d_rn_, reinterpret_cast<const uint4*>(d_hdr_), d_rec_,
                       reinterpret_cast<uint2*>(d_plframes), closing_plsc);
    return launched("pl framer kernel launch");
}

} // namespace dvbs2
