// bbframer_hip.hip -- see bbframer_hip.h. ONE launch per call, bbf_frame_kernel:
//   The output of the call is ONE flat byte array, cut into tiles of 4096 bytes on 16-byte boundaries of the output ADDRESS (kbch / 8 is
//   odd for many rows: a frame is not even 2-byte aligned). The DATAFIELDs of consecutive frames continue each other in E, so a tile
//   needs one contiguous piece of E. A workgroup
//     1  stages that piece in LDS as aligned dwords of the input, the carried tail in front of it;
//     2  works out the CRC slots that fall into the piece (at most 22): sixteen lanes per packet, each lane runs the table CRC over its
//        twelve bytes, multiplies by x^(8 * distance to the end) mod g, and the sixteen XOR-reduce with __shfl_xor; the sync bytes
//        are checked here (sync_errors);
//     3  patches the slots into the image;
//     4  builds one 16-byte piece of the output per lane -- a funnel shift of five LDS dwords inside a DATAFIELD, zeros inside the
//        padding, byte by byte where a header, a field boundary or an end of the output falls into the piece.
//   The handle keeps TWO copies of the carried state and the host alternates them: every workgroup reads the copy the call before
//   wrote, the last workgroup writes the other one (the last packet of the call, its CRC, the counters). sync_errors is only ever
//   added to atomically and lives beside them.
#include <cstdlib>
#include "bbframer_hip.h"
#include "crc8_dev.h"

namespace dvbs2 {

// r * x^8 mod x^8 + x^7 + x^6 + x^4 + x^2 + 1 (r < 256)
__host__ __device__ constexpr uint32_t gf_mulx8(uint32_t r)
{
    r <<= 8;
    for (int b = 15; b >= 8; b--) if (r & (1u << b)) r ^= 0x1D5u << (b - 8);
    return r;
}

/* ------------------------------------------------------------------ host only */
int crc8(const uint8_t* data, size_t n)
{
    uint32_t reg = 0;
    for (size_t i = 0; i < n; i++) reg = gf_mulx8(reg) ^ data[i];
    return (int)gf_mulx8(reg);
}

int bbheader_build(uint8_t out[10], int matype1, int matype2, int upl_bits, int dfl_bits, int sync, int syncd_bits)
{
    if ((matype1 | matype2 | sync) & ~0xff || (upl_bits | dfl_bits | syncd_bits) & ~0xffff) return -1; // (a negative value has high bits)
    const uint8_t h[9] = { (uint8_t)matype1, (uint8_t)matype2, (uint8_t)(upl_bits >> 8), (uint8_t)upl_bits, (uint8_t)(dfl_bits >> 8),
                           (uint8_t)dfl_bits, (uint8_t)sync, (uint8_t)(syncd_bits >> 8), (uint8_t)syncd_bits };
    for (int i = 0; i < 9; i++) out[i] = h[i];
    out[9] = (uint8_t)crc8(h, 9);
    return 0;
}

int64_t bbframer_need(uint64_t pos, int n_frames, int dfl_bytes)
{
    const uint64_t end = pos + (uint64_t)n_frames * (uint64_t)dfl_bytes;
    return (int64_t)((end + kBbfTsLen - 1) / kBbfTsLen - (pos + kBbfTsLen - 1) / kBbfTsLen);
}

std::string bbframer_check_create(int kbch_bits, int max_frames)
{
    if (kbch_bits < 88 || kbch_bits % 8 != 0 || kbch_bits - 80 > 0xffff) return "kbch_bits: unsupported BCH message length";
    if (kbch_bits / 8 - kBbfHeaderBytes < kBbfTsLen) return "kbch_bits: max_dfl_bytes is below one TS packet";
    if (max_frames < 1 || max_frames > 65535) return "max_frames must be in 1..65535";
    return "";
}

int bbframer_check_call(int max_frames, int max_dfl_bytes, int n_frames, int dfl_bytes, std::string* text)
{
    if (n_frames < 0 || n_frames > max_frames) { *text = "n_frames must be in 0..max_frames"; return kSize; }
    if (dfl_bytes != 0 && (dfl_bytes < kBbfTsLen || dfl_bytes > max_dfl_bytes)) { *text = "dfl_bytes must be 0 or in 188..max_dfl_bytes"; return kArgument; }
    return 0;
}

/* ------------------------------------------------------------------ device */
// x^(8 * (188 - i)) mod g for byte i of a packet: what byte i weighs in the check byte of bytes 1..187; byte 0 and the pad weigh nothing
struct BbfPowers { uint8_t v[192]; };
constexpr BbfPowers bbf_make_powers()
{
    BbfPowers p{};
    uint32_t r = 1;
    for (int i = kBbfTsLen - 1; i >= 1; i--) { r = gf_mulx8(r); p.v[i] = (uint8_t)r; }
    return p;
}
__constant__ BbfPowers kBbfPow = bbf_make_powers();

// a * b mod g (both < 256)
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        r <<= 1;
        if (r & 0x100u) r ^= 0x1D5u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// The four bytes t .. t + 3 of the call's input, little endian; in + t is 4-byte aligned. A dword that lies inside the input is one
// aligned load; one that sticks out is put together from the bytes that exist: before the input from `carry` (the last packet of the
// call before, t = -1 is its byte 187; null: zeros), behind it zeros. Nothing outside [in, in + n_in) is read.
__device__ __forceinline__ uint32_t bbf_load4(const uint8_t* __restrict__ in, int n_in, int t, const uint8_t* __restrict__ carry)
{
    if (t >= 0 && t + 4 <= n_in) return *reinterpret_cast<const uint32_t*>(in + t);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int u = t + j;
        uint32_t b = 0;
        if (u >= 0 && u < n_in) b = in[u];
        else if (u < 0 && u >= -kBbfTsLen && carry) b = carry[kBbfTsLen + u];
        v |= b << (8 * j);
    }
    return v;
}

constexpr int kBbfAsmThreads = 256, kBbfPiece = 16, kBbfTile = kBbfAsmThreads * kBbfPiece;

struct BbfCall { // one call, by value. Offsets are ints: a call writes at most 65535 * 8201 bytes
    const uint8_t* in; int n_in;   // the packets of the call, bytes
    int n_pkts;
    uint8_t* out16; int lead;      // the output starts `lead` bytes behind out16, which is 16-byte aligned
    int total;                     // n_frames * kbch_bytes
    int n_frames, kbch_bytes, dfl;
    int t0;                        // where frame 0's DATAFIELD starts in E, as a byte offset into `in`: -(carried bytes), in (-188, 0]
    int r0;                        // pos % 188
    int first;                     // no packet was presented before this call: the byte at offset 0 is packet 0's own sync byte
    int serial;                    // measurement only: one lane per CRC, 187 dependent table steps
    uint8_t h[7]; uint8_t reg7;    // the seven header bytes before SYNCD and the CRC register after them
};

// offset into `in` of the first DATAFIELD byte at or behind output offset o (o in 0..total)
__device__ __forceinline__ int bbf_t_of(const BbfCall& c, int o)
{
    const int f = o / c.kbch_bytes, w = o - f * c.kbch_bytes;
    return c.t0 + f * c.dfl + min(max(w - kBbfHeaderBytes, 0), c.dfl);
}

// byte o of the output, the general way
__device__ uint32_t bbf_byte_at(const BbfCall& c, int o, const uint32_t* img, int t_base)
{
    const int f = o / c.kbch_bytes, w = o - f * c.kbch_bytes;
    if (w >= kBbfHeaderBytes + c.dfl) return 0;
    if (w >= kBbfHeaderBytes) return reinterpret_cast<const uint8_t*>(img)[c.t0 + f * c.dfl + (w - kBbfHeaderBytes) - t_base];
    if (w < 7) return c.h[w];
    const uint32_t s = ((uint32_t)c.r0 + (uint32_t)f * (uint32_t)c.dfl) % kBbfTsLen; // frames * dfl < 2^30
    const uint32_t syncd = 8u * ((kBbfTsLen - s) % kBbfTsLen);
    if (w == 7) return syncd >> 8;
    if (w == 8) return syncd & 0xffu;
    return gf_mulx8(gf_mulx8(gf_mulx8(c.reg7) ^ (syncd >> 8)) ^ (syncd & 0xffu));
}

// the aligned dword of the input at offset t, from the image where it holds it (only bytes at offsets >= 0 are asked for)
__device__ __forceinline__ uint32_t bbf_dword(const BbfCall& c, const uint32_t* img, int t_base, int n_dw, int t)
{
    const int k = (t - t_base) >> 2;
    if (t >= t_base && k < n_dw) return img[k];
    return bbf_load4(c.in, c.n_in, t, nullptr);
}

__global__ __launch_bounds__(kBbfAsmThreads) void bbf_frame_kernel(const BbfCall c, const BbfState* __restrict__ cur, BbfState* __restrict__ nxt,
                                                                   unsigned long long* __restrict__ sync_errors)
{
    __shared__ uint32_t img[kBbfTile / 4 + 8]; // the tile's piece of E, from an aligned dword of the input on
    __shared__ uint8_t tab[256];
    __shared__ uint8_t job_crc[32];
    const int tid = threadIdx.x;
    const int o_lo = (int)blockIdx.x * kBbfTile - c.lead; // output offset of the tile's first byte (negative inside the lead)
    const int lo = max(o_lo, 0), hi = min(o_lo + kBbfTile, c.total);
    const int t_lo = bbf_t_of(c, lo), t_hi = bbf_t_of(c, hi);
    const int t_base = t_lo - (int)(((uintptr_t)c.in + (uintptr_t)(intptr_t)t_lo) & 3);
    const int n_dw = (t_hi - t_base + 3) >> 2; // <= (4096 + 3 + 3) / 4
    crc8_build(tab, tid, kBbfAsmThreads);
    for (int k = tid; k < n_dw; k += kBbfAsmThreads) img[k] = bbf_load4(c.in, c.n_in, t_base + 4 * k, cur->last_pkt);
    __syncthreads();
    // The CRC slots of the piece: offsets 188 q in [t_lo, t_hi), at most 22. Job j < n_slots is the CRC of packet q_first + j - 1 for
    // the slot of packet q_first + j (q = 0: the carried CRC, nothing to do); the last workgroup has one job more, the CRC of the
    // last packet of the call for the next call.
    const int q_first = t_lo <= 0 ? 0 : (t_lo + kBbfTsLen - 1) / kBbfTsLen;
    const int n_slots = t_hi > q_first * kBbfTsLen ? (t_hi - q_first * kBbfTsLen + kBbfTsLen - 1) / kBbfTsLen : 0;
    const bool last = blockIdx.x == gridDim.x - 1;
    const int n_jobs = n_slots + (last ? 1 : 0);
    const int a = (int)((uintptr_t)c.in & 3); // every packet starts at this phase of a dword: 188 = 4 * 47
    if (!c.serial) {
        for (int j0 = 0; j0 < n_jobs; j0 += kBbfAsmThreads / 16) { // (the same trips for every lane: the shuffles below)
            const int j = j0 + (tid >> 4), l = tid & 15;
            const int p = j < n_slots ? q_first + j - 1 : (j < n_jobs ? c.n_pkts - 1 : -1);
            uint32_t acc = 0;
            if (p >= 0) { // lane l: the three aligned dwords that hold packet bytes 12 l - a .. 12 l - a + 11
                uint32_t reg = 0;
                int i1 = 0;
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const int i0 = 4 * (3 * l + d) - a;
                    const uint32_t w = bbf_dword(c, img, t_base, n_dw, p * kBbfTsLen + i0);
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int i = i0 + b;
                        if (i >= 1 && i < kBbfTsLen) { reg = crc8_step(reg, (w >> (8 * b)) & 0xffu, tab); i1 = i; }
                    }
                }
                if (i1) acc = gf_mul(reg, kBbfPow.v[i1]); // the lane's bytes end at byte i1
            }
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) acc ^= __shfl_xor(acc, m);
            if (l == 0 && p >= 0) job_crc[j] = (uint8_t)acc;
        }
    } else if (tid < n_jobs) {
        const int p = tid < n_slots ? q_first + tid - 1 : c.n_pkts - 1;
        if (p >= 0) {
            uint32_t reg = 0;
            for (int i = 1; i < kBbfTsLen; i++) {
                const int t = p * kBbfTsLen + i, ta = t - ((a + i) & 3); // (in + ta is aligned: t = i mod 4)
                reg = crc8_step(reg, (bbf_dword(c, img, t_base, n_dw, ta) >> (8 * (t - ta))) & 0xffu, tab);
            }
            job_crc[tid] = tab[reg];
        }
    }
    __syncthreads();
    if (tid < n_slots) { // the sync byte of packet q is checked, then its slot takes the CRC of the packet before
        const int q = q_first + tid;
        uint8_t* slot = reinterpret_cast<uint8_t*>(img) + (q * kBbfTsLen - t_base);
        if (*slot != 0x47) atomicAdd(sync_errors, 1ull);
        if (q >= 1) *slot = job_crc[tid];
        else if (!c.first) *slot = cur->last_crc;
    }
    if (last) { // for the next call, into the copy nobody reads in this launch
        if (tid < kBbfTsLen) nxt->last_pkt[tid] = c.in[(size_t)(c.n_pkts - 1) * kBbfTsLen + tid];
        if (tid == 0) {
            nxt->last_crc = job_crc[n_slots];
            nxt->packets = cur->packets + (unsigned long long)c.n_pkts;
            nxt->bbframes = cur->bbframes + (unsigned long long)c.n_frames;
        }
    }
    __syncthreads();
    const int o0 = o_lo + kBbfPiece * tid;
    if (o0 >= c.total || o0 + kBbfPiece <= 0) return;
    uint8_t* dst = c.out16 + (size_t)blockIdx.x * kBbfTile + kBbfPiece * tid;
    const bool whole = o0 >= 0 && o0 + kBbfPiece <= c.total;
    if (whole) {
        const int f = o0 / c.kbch_bytes, w = o0 - f * c.kbch_bytes;
        if (w >= kBbfHeaderBytes && w + kBbfPiece <= kBbfHeaderBytes + c.dfl) { // inside a DATAFIELD
            const int bi = c.t0 + f * c.dfl + (w - kBbfHeaderBytes) - t_base, k = bi >> 2, sh = 8 * (bi & 3);
            uint32_t d[5];
#pragma unroll
            for (int j = 0; j < 5; j++) d[j] = img[k + j]; // (the fifth counts only with a shift; it lies inside img either way)
            uint4 v;
            v.x = (uint32_t)((((uint64_t)d[1] << 32) | d[0]) >> sh);
            v.y = (uint32_t)((((uint64_t)d[2] << 32) | d[1]) >> sh);
            v.z = (uint32_t)((((uint64_t)d[3] << 32) | d[2]) >> sh);
            v.w = (uint32_t)((((uint64_t)d[4] << 32) | d[3]) >> sh);
            *reinterpret_cast<uint4*>(dst) = v;
            return;
        }
        if (w >= kBbfHeaderBytes + c.dfl && w + kBbfPiece <= c.kbch_bytes) { // inside the padding
            *reinterpret_cast<uint4*>(dst) = make_uint4(0, 0, 0, 0);
            return;
        }
    }
    // a header, a field boundary or an end of the output falls into the piece
    uint32_t v[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int j = 0; j < kBbfPiece; j++) {
        const int o = o0 + j;
        if (o >= 0 && o < c.total) v[j >> 2] |= bbf_byte_at(c, o, img, t_base) << (8 * (j & 3));
    }
    if (whole) { *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]); return; }
#pragma unroll
    for (int j = 0; j < kBbfPiece; j++) {
        const int o = o0 + j;
        if (o >= 0 && o < c.total) dst[j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
    }
}

/* ------------------------------------------------------------------ the stage */
BbFramerHip::BbFramerHip(int kbch_bits, int max_frames, int device) : DeviceStage(device), kbch_bytes_(kbch_bits / 8), max_frames_(max_frames)
{
    const std::string bad = bbframer_check_create(kbch_bits, max_frames);
    if (!bad.empty()) { err_.argument(bad); return; }
    if (const char* e = getenv("DVBS2_BBFRAMER_CRC")) crc_serial_ = std::string(e) == "serial"; // measurement only
    DeviceGuard guard(device_);
    if (!guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc of the bbframer state", alloc(&d_, 1));
    HIP_OK(memset_done(d_, 0, sizeof(BbfDevice)));
}

int BbFramerHip::set_matype(int matype1, int matype2)
{
    call_err_ = {};
    if (matype1 < 0 || matype1 > 255) { call_err_.argument("matype1 must be in 0..255"); return -1; }
    if (matype2 < 0 || matype2 > 255) { call_err_.argument("matype2 must be in 0..255"); return -1; }
    matype1_ = matype1; matype2_ = matype2;
    return 0;
}

int BbFramerHip::need(int n_frames, int dfl_bytes, int* n_packets)
{
    call_err_ = {};
    std::string text;
    if (const int code = bbframer_check_call(max_frames_, max_dfl_bytes(), n_frames, dfl_bytes, &text)) { call_err_ = { code, text }; return -1; }
    if (n_packets) *n_packets = (int)bbframer_need(pos_, n_frames, dfl_bytes ? dfl_bytes : max_dfl_bytes());
    return 0;
}

int BbFramerHip::process_device(const uint8_t* d_ts, int n_frames, int dfl_bytes, uint8_t* d_bbframes, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    int n_pkts = 0;
    if (need(n_frames, dfl_bytes, &n_pkts)) return -1;
    if (n_frames == 0) return 0;
    if (!d_ts) { call_err_.argument("d_ts is null"); return -1; }
    if (!d_bbframes) { call_err_.argument("d_bbframes is null"); return -1; }
    const int dfl = dfl_bytes ? dfl_bytes : max_dfl_bytes();
    BbfCall c;
    c.in = d_ts; c.n_in = n_pkts * kBbfTsLen; // (a call of a frame or more reads a packet or more: dfl >= 188 > the carried tail)
    c.total = n_frames * kbch_bytes_;
    const uintptr_t a = (uintptr_t)d_ts, b = (uintptr_t)d_bbframes;
    if (a < b + (uintptr_t)c.total && b < a + (uintptr_t)c.n_in) { call_err_.argument("d_ts and d_bbframes overlap"); return -1; }
    c.lead = (int)(b & 15); c.out16 = d_bbframes - c.lead;
    c.kbch_bytes = kbch_bytes_; c.dfl = dfl;
    c.r0 = (int)(pos_ % kBbfTsLen); c.t0 = -((kBbfTsLen - c.r0) % kBbfTsLen); c.first = pos_ == 0;
    uint8_t h[10];
    bbheader_build(h, matype1_, matype2_, kBbfTsLen * 8, dfl * 8, 0x47, 0);
    uint32_t reg = 0;
    for (int i = 0; i < 7; i++) { c.h[i] = h[i]; reg = gf_mulx8(reg) ^ h[i]; }
    c.reg7 = (uint8_t)reg;
    c.n_pkts = n_pkts; c.n_frames = n_frames; c.serial = crc_serial_;
    hipLaunchKernelGGL(bbf_frame_kernel, dim3((c.lead + c.total + kBbfTile - 1) / kBbfTile), dim3(kBbfAsmThreads), 0, stream, c, &d_->st[cur_], &d_->st[cur_ ^ 1],
                       &d_->sync_errors);
    if (launched("bbframer launch")) return -1;
    pos_ += (uint64_t)n_frames * (uint64_t)dfl;
    cur_ ^= 1;
    return 0;
}

int BbFramerHip::counters(BbfCounters* out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    BbfState st;
    unsigned long long sync_errors = 0;
    hipError_t e = hipMemcpyAsync(&st, &d_->st[cur_], sizeof(BbfState), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&sync_errors, &d_->sync_errors, sizeof(sync_errors), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (!hip_ok(e, "bbframer counters", call_err_)) return -1;
    out->packets = st.packets; out->bbframes = st.bbframes; out->sync_errors = sync_errors;
    return 0;
}

int BbFramerHip::reset(hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (!hip_ok(hipMemsetAsync(d_, 0, sizeof(BbfDevice), stream), "bbframer reset", call_err_)) return -1;
    pos_ = 0; cur_ = 0;
    return 0;
}

} // namespace dvbs2
