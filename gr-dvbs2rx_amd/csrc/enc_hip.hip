// enc_hip.hip -- BBFRAME bytes -> BCH codeword -> LDPC codeword -> XFECFRAME symbols on gfx950: the inverse of the decode chain, all
// integer work and table look-ups, every result bit for bit (notes/encoder.md).
//
//   BCH     one workgroup of 256 threads per frame. The remainder of m(x) x^(n-k) mod g(x) is linear in the message: thread t runs the
//           byte-wise shift register (one 256-entry table of 192-bit values in LDS) over its own segment of L message bytes, and a
//           binary tree joins the 256 segment remainders: left * x^(8 L 2^j) mod g + right at level j, the multiplication a 192 x 192
//           bit matrix per level, precomputed by the host. One path for every batch size. The BB scrambler is an xor in the load.
//   LDPC    one workgroup per frame, the information bits in LDS. Address x = a q + b of group g feeds parity ((a + m) mod 360) q + b
//           from information bit 360 g + m: thread t (0 .. 359) owns the q consecutive parity bits t q .. t q + q - 1, i.e. residue
//           b = 0 .. q - 1 of row t, and reads information bit 360 g + (t - a) mod 360 for every entry of the residue. The running xor
//           over the bits of a thread is the accumulate rule p[r] ^= p[r - 1] inside its run; the xor of everything before the run
//           comes from a prefix over the 360 row totals (wave ballots) and flips the whole run.
//   mapper  one thread per two symbols (one 16-byte store): label bits gathered through the column layout, the point copied from a
//           table of at most 256 entries in LDS.
#include "enc_hip.h"
#include "demap_hip.h"
#include "../../include/dvbs2_fec_hip.h"
#include <algorithm>
#include <array>
#include <cstring>

namespace dvbs2 {

constexpr int kEncBchThreads = 256, kEncBchLevels = 8; // 2^8 segments
constexpr int kEncRemWords = 6;                        // deg g <= 192
constexpr int kEncMaxBytes = 7296;                     // message / information bytes of a frame: K <= 58320 bits
constexpr int kEncLdpcThreads = 384;                   // 360 rows, six waves
constexpr int kEncParWords = 1576;                     // N - K <= 50400 bits (2/9 normal)

struct EncBchArgs {
    const uint8_t* in; uint8_t* cw; const uint8_t* scramble; // scramble: k/8 bytes of the BB PRBS or nullptr
    const uint32_t* tab;  // [6][256]: word w of (v(x) x^r mod g), coefficient of x^(r-1) in bit 31 of word 0
    const uint32_t* join; // [level][bit position p][6]: x^(r-1-p + 8 L 2^level) mod g
    int kb, nb, seg;      // message bytes, codeword bytes, L
};

__global__ __launch_bounds__(kEncBchThreads) void enc_bch_kernel(const EncBchArgs a)
{
    __shared__ uint32_t tab[kEncRemWords][256];
    __shared__ uint32_t rem[kEncBchThreads][kEncRemWords];
    __shared__ uint8_t msg[kEncMaxBytes];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
#pragma unroll
    for (int w = 0; w < kEncRemWords; w++) tab[w][tid] = a.tab[w * 256 + tid];
    const uint8_t* in = a.in + f * (size_t)a.kb;
    uint8_t* out = a.cw + f * (size_t)a.nb;
    for (int b = tid; b < a.kb; b += kEncBchThreads) { // (bbscrambler fused: in ^= PRBS)
        const uint8_t v = a.scramble ? (uint8_t)(in[b] ^ a.scramble[b]) : in[b];
        msg[b] = v; out[b] = v;
    }
    __syncthreads();
    // the message with zero bytes in front so that 256 segments of L bytes cover it: leading zeros do not change a remainder
    const int start = tid * a.seg - (kEncBchThreads * a.seg - a.kb);
    uint32_t r[kEncRemWords];
#pragma unroll
    for (int w = 0; w < kEncRemWords; w++) r[w] = 0;
    for (int i = 0; i < a.seg; i++) {
        const int at = start + i;
        const uint32_t byte = at >= 0 ? (uint32_t)msg[at] : 0u;
        const uint32_t idx = (r[0] >> 24) ^ byte;
#pragma unroll
        for (int w = 0; w < kEncRemWords; w++) r[w] = ((r[w] << 8) | (w + 1 < kEncRemWords ? r[w + 1] >> 24 : 0u)) ^ tab[w][idx];
    }
#pragma unroll
    for (int w = 0; w < kEncRemWords; w++) rem[tid][w] = r[w];
    for (int lv = 0; lv < kEncBchLevels; lv++) {
        __syncthreads();
        if ((tid & ((2 << lv) - 1)) == 0) {
            uint32_t acc[kEncRemWords];
#pragma unroll
            for (int w = 0; w < kEncRemWords; w++) acc[w] = rem[tid + (1 << lv)][w];
            const uint32_t* jm = a.join + (size_t)lv * 192 * kEncRemWords;
#pragma unroll
            for (int w = 0; w < kEncRemWords; w++) {
                uint32_t bits = rem[tid][w];
                while (bits) {
                    const int p = __clz((int)bits);
                    bits &= ~(0x80000000u >> p);
                    const uint32_t* row = jm + (size_t)(32 * w + p) * kEncRemWords;
#pragma unroll
                    for (int x = 0; x < kEncRemWords; x++) acc[x] ^= row[x];
                }
            }
#pragma unroll
            for (int w = 0; w < kEncRemWords; w++) rem[tid][w] = acc[w];
        }
    }
    __syncthreads();
    if (tid < a.nb - a.kb) out[a.kb + tid] = (uint8_t)(rem[0][tid >> 2] >> (24 - 8 * (tid & 3))); // highest power first
}

struct EncLdpcArgs {
    const uint8_t* in; uint8_t* cw;
    const uint32_t* off; const uint32_t* ent; // residue b: entries off[b] .. off[b + 1], each (360 g) << 9 | a
    int kb, nb, q;
};

__global__ __launch_bounds__(kEncLdpcThreads) void enc_ldpc_kernel(const EncLdpcArgs a)
{
    __shared__ uint8_t info[kEncMaxBytes];
    __shared__ uint32_t par[kEncParWords]; // parity bit r in bit 31 - (r & 31) of word r >> 5
    __shared__ unsigned long long totals[kEncLdpcThreads / 64];
    const int tid = threadIdx.x, q = a.q;
    const size_t f = blockIdx.x;
    const uint8_t* in = a.in + f * (size_t)a.kb;
    uint8_t* out = a.cw + f * (size_t)a.nb;
    const int pb = a.nb - a.kb, pw = (8 * pb + 31) / 32;
    for (int b = tid; b < a.kb; b += kEncLdpcThreads) { const uint8_t v = in[b]; info[b] = v; out[b] = v; }
    for (int w = tid; w < pw; w += kEncLdpcThreads) par[w] = 0;
    __syncthreads();
    const bool row = tid < 360;
    const int first = tid * q; // this thread's run of parity bits: first .. first + q - 1
    uint32_t run = 0;
    if (row) {
        int word = first >> 5;
        uint32_t accw = 0;
        for (int b = 0; b < q; b++) {
            uint32_t bit = 0;
            const uint32_t e1 = a.off[b + 1];
            for (uint32_t e = a.off[b]; e < e1; e++) {
                const uint32_t en = a.ent[e];
                int m = tid - (int)(en & 511u);
                m += m < 0 ? 360 : 0;
                const uint32_t idx = (en >> 9) + (uint32_t)m;
                bit ^= (uint32_t)info[idx >> 3] >> (7 - (idx & 7));
            }
            run ^= bit & 1u;
            const int r = first + b;
            if ((r >> 5) != word) { if (accw) atomicXor(&par[word], accw); accw = 0; word = r >> 5; }
            accw |= run << (31 - (r & 31));
        }
        if (accw) atomicXor(&par[word], accw);
    }
    // p[r] ^= p[r - 1] across the runs: the xor of the totals of all earlier rows flips every bit of this row's run
    const unsigned long long ball = __ballot(row && run);
    if ((tid & 63) == 0) totals[tid >> 6] = ball;
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(ball & ((1ull << (tid & 63)) - 1ull));
    for (int w = 0; w < (tid >> 6); w++) before += (uint32_t)__popcll(totals[w]);
    if (row && (before & 1u)) {
        int r = first;
        const int end = first + q;
        while (r < end) {
            const int n = min(32 - (r & 31), end - r); // bits r .. r + n - 1 of one word
            const uint32_t mask = (n == 32 ? 0xffffffffu : ((1u << n) - 1u) << (32 - (r & 31) - n));
            atomicXor(&par[r >> 5], mask);
            r += n;
        }
    }
    __syncthreads();
    for (int j = tid; j < pb; j += kEncLdpcThreads) out[a.kb + j] = (uint8_t)(par[j >> 2] >> (24 - 8 * (j & 3)));
}

struct EncMapArgs {
    const uint8_t* cw; float* syms; const float2* points;
    int n_syms, step, nb;
    int base[8], shift[8];
    unsigned long long total; // symbols of the batch
};

template <int NMOD>
__global__ __launch_bounds__(256) void enc_map_kernel(const EncMapArgs a)
{
    __shared__ float2 tab[1 << NMOD];
    for (int i = threadIdx.x; i < (1 << NMOD); i += 256) tab[i] = a.points[i];
    __syncthreads();
    const float inv_n = 1.0f / (float)a.n_syms;
    auto point = [&](unsigned long long s64) -> float2 {
        // frame = s / n_syms without an integer division: s < 65535 * 32400 < 2^31, the float quotient is off by at most one
        // (an error of 2^-23 relative, n_syms >= 2025) and the two comparisons below settle it
        const uint32_t s = (uint32_t)s64, n = (uint32_t)a.n_syms;
        uint32_t f = (uint32_t)((float)s * inv_n);
        if (f * n > s) f--;
        if ((f + 1) * n <= s) f++;
        const int j = (int)(s - f * n);
        const uint8_t* cw = a.cw + f * (size_t)a.nb;
        uint32_t idx = 0;
#pragma unroll
        for (int c = 0; c < NMOD; c++) {
            const int bi = a.base[c] + a.step * j;
            idx |= (((uint32_t)cw[bi >> 3] >> (7 - (bi & 7))) & 1u) << a.shift[c];
        }
        return tab[idx];
    };
    const bool wide = ((uintptr_t)a.syms & 15) == 0;
    const unsigned long long pairs = (a.total + 1) / 2;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long s = 2 * i;
        const float2 p0 = point(s);
        if (s + 1 < a.total) {
            const float2 p1 = point(s + 1);
            if (wide) reinterpret_cast<float4*>(a.syms)[i] = make_float4(p0.x, p0.y, p1.x, p1.y);
            else { reinterpret_cast<float2*>(a.syms)[s] = p0; reinterpret_cast<float2*>(a.syms)[s + 1] = p1; }
        } else
            reinterpret_cast<float2*>(a.syms)[s] = p0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host: the verdict
static void enc_bch_field(int framesize, int* m, uint32_t* prim)
{   // reference lib/bch_decoder_bb_impl.cc:58-63
    if (framesize == DVBS2_FECFRAME_NORMAL) { *m = 16; *prim = 0x1002Du; }
    else if (framesize == DVBS2_FECFRAME_SHORT) { *m = 14; *prim = 0x402Bu; }
    else { *m = 15; *prim = 0x802Du; }
}

static void enc_columns(EncMapper* map, int n_mod, int n_syms, const uint8_t* column)
{
    map->n_mod = n_mod; map->step = 1;
    for (int c = 0; c < n_mod; c++) { map->base[c] = c * n_syms; map->shift[c] = n_mod - 1 - (column ? column[c] : c); }
}

bool enc_table_mapper(int N, int n_mod, const float* points_re_im, const uint8_t* column, EncMapper* map, std::string* why)
{
    if (!demap_table_check(n_mod, points_re_im, column, why)) return false;
    if (N % n_mod) { *why = "n_mod: the frame length " + std::to_string(N) + " is not a multiple of " + std::to_string(n_mod); return false; }
    enc_columns(map, n_mod, N / n_mod, column);
    map->points.assign(points_re_im, points_re_im + (2 << n_mod));
    return true;
}

bool enc_spec(int standard, int framesize, int rate, int constellation, EncSpec* spec, std::string* why)
{
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi) || !fi.table) { *why = "unsupported (standard, framesize, rate)"; return false; }
    if ((int)fi.bch_n != fi.table->K) {
        *why = "rate: bch_n " + std::to_string(fi.bch_n) + " != table K " + std::to_string(fi.table->K) + " of " + fi.table->name +
               " (a shortened / punctured VL-SNR or medium row: its pattern is not pinned by the reference; dvbs2_enc_create_parts encodes the mother code)";
        return false;
    }
    if (fi.bch_n % 8 || fi.bch_k % 8) { *why = "framesize: u8 array messages are only supported for n and k multiple of 8."; return false; }
    EncSpec s;
    enc_bch_field(framesize, &s.bch_m, &s.bch_prim);
    s.bch_t = (int)fi.bch_t; s.bch_n = (int)fi.bch_n;
    s.table = fi.table;
    const int N = fi.table->N;
    if (constellation == DVBS2_ENC_NO_MAPPER || constellation == kEncCallerTable) { *spec = s; return true; }
    if (constellation != DVBS2_MOD_QPSK && constellation != DVBS2_MOD_8PSK && constellation != DVBS2_MOD_16APSK && constellation != DVBS2_MOD_32APSK) {
        *why = "constellation: Unsupported constellation (DVBS2_MOD_QPSK, _8PSK, _16APSK, _32APSK or DVBS2_ENC_NO_MAPPER)"; return false;
    }
    if (standard != DVBS2_STANDARD_DVBS2) { *why = "constellation: a DVB-T2 rate has no built-in mapper (DVBS2_ENC_NO_MAPPER or a caller's table)"; return false; }
    EncMapper& mp = s.map;
    if (constellation == DVBS2_MOD_QPSK) { // bit 2 j -> I, 2 j + 1 -> Q, bit 0 positive
        const float a = 0.70710678118654752440f;
        mp.n_mod = 2; mp.step = 2; mp.base[0] = 0; mp.base[1] = 1; mp.shift[0] = 1; mp.shift[1] = 0;
        mp.points = { a, a, a, -a, -a, a, -a, -a };
    } else if (constellation == DVBS2_MOD_8PSK) { // the point the demapper's refinement re-maps from b0 b1 b2 (demap_snr_kernel)
        const float a = 0.70710678118654752440f;
        const int rows = N / 3;
        int order = 0; // as DemapperHip: C3_5 = 4 "210"; C25_36, C13_18, C7_15, C8_15, C26_45 "102"
        if (rate == 4) order = 1;
        else if (rate == 26 || rate == 28 || rate == 38 || rate == 39 || rate == 19) order = 2;
        mp.n_mod = 3; mp.step = 1;
        mp.base[0] = 0; mp.base[1] = rows; mp.base[2] = 2 * rows;
        if (order == 1) { mp.base[0] = 2 * rows; mp.base[1] = rows; mp.base[2] = 0; }
        else if (order == 2) { mp.base[0] = rows; mp.base[1] = 0; mp.base[2] = 2 * rows; }
        mp.shift[0] = 2; mp.shift[1] = 1; mp.shift[2] = 0;
        mp.points = { a, a, 1, 0, -1, 0, -a, -a, 0, 1, a, -a, -a, a, -0.0f, -1 }; // (the last point is -1j: its real part is -0)
    } else {
        const int n_mod = constellation == DVBS2_MOD_16APSK ? 4 : 5;
        float p[64];
        if (framesize == DVBS2_FECFRAME_MEDIUM) { *why = "framesize: Unsupported frame size for 16APSK / 32APSK (normal and short only)"; return false; }
        if (!apsk_points(constellation, rate, p) || (rate == 11 && framesize != DVBS2_FECFRAME_NORMAL)) {
            *why = "constellation: Unsupported code rate for 16APSK / 32APSK (DVB-S2: 16APSK 2/3 .. 9/10, 32APSK 3/4 .. 9/10; 9/10 normal frames only)";
            return false;
        }
        enc_columns(&mp, n_mod, N / n_mod, nullptr);
        mp.points.assign(p, p + (2 << n_mod));
    }
    *spec = s;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- host: the plans
namespace {
using Rem = std::array<uint32_t, kEncRemWords>;
// remainders are kept left-aligned: the coefficient of x^(r-1) is bit 31 of word 0, whatever r = deg g is
struct RemRing {
    Rem g{}; // g(x) without its leading term
    explicit RemRing(const BchCode& c)
    {
        for (int i = 0; i < c.gdeg; i++) if (c.gen[i]) { const int p = c.gdeg - 1 - i; g[p >> 5] |= 0x80000000u >> (p & 31); }
    }
    void shift_in(Rem& r, uint32_t bit) const // r = r x + bit x^deg, mod g
    {
        const uint32_t fb = (r[0] >> 31) ^ bit;
        for (int w = 0; w < kEncRemWords; w++) r[w] = (r[w] << 1) | (w + 1 < kEncRemWords ? r[w + 1] >> 31 : 0u);
        if (fb) for (int w = 0; w < kEncRemWords; w++) r[w] ^= g[w];
    }
};
} // namespace

EncoderHip::EncoderHip(const EncSpec& spec, int max_frames, int device) : DeviceStage(device), max_frames_(max_frames)
{
    has_bch_ = spec.bch_m != 0; has_ldpc_ = spec.table != nullptr;
    if (!has_bch_ && !has_ldpc_) { err_.argument("at least one of the BCH and the LDPC stage is required"); return; }
    if (has_bch_) {
        if (std::string bad; !code_.build(spec.bch_m, spec.bch_prim, spec.bch_t, spec.bch_n, &bad)) { err_.argument(bad); return; }
        if (code_.n % 8 || code_.k % 8) { err_.argument("u8 array messages are only supported for n and k multiple of 8."); return; } // lib/bch.cc:19-24
        if (code_.gdeg > 32 * kEncRemWords || code_.k / 8 > kEncMaxBytes) { err_.argument("BCH code beyond the encoder's limits (deg g <= 192, k <= 58368)"); return; }
    }
    if (has_ldpc_) {
        N_ = spec.table->N; K_ = spec.table->K; q_ = (N_ - K_) / 360;
        if (K_ / 8 > kEncMaxBytes || (N_ - K_ + 31) / 32 > kEncParWords) { err_.argument("LDPC table beyond the encoder's limits"); return; }
        if (has_bch_ && code_.n != K_) { err_.argument("bch_n " + std::to_string(code_.n) + " != table K " + std::to_string(K_) + " of " + spec.table->name); return; }
    }
    map_ = spec.map;
    if (map_.n_mod && !has_ldpc_) { err_.argument("a mapper needs the LDPC stage"); return; }
    if (max_frames_ < 1 || max_frames_ > 65535) { err_.argument("max_frames must be in 1..65535 (frames are one launch dimension)"); return; }
    DeviceGuard dev_guard(device_);
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    if (has_bch_) {
        const RemRing ring(code_);
        std::vector<uint32_t> tab(kEncRemWords * 256);
        for (uint32_t v = 0; v < 256; v++) { // v(x) x^r mod g
            Rem r{};
            for (int b = 7; b >= 0; b--) ring.shift_in(r, (v >> b) & 1u);
            for (int w = 0; w < kEncRemWords; w++) tab[w * 256 + v] = r[w];
        }
        const int kb = code_.k / 8;
        bch_seg_ = (kb + kEncBchThreads - 1) / kEncBchThreads;
        std::vector<uint32_t> join((size_t)kEncBchLevels * 192 * kEncRemWords, 0);
        Rem v{}; // x^s mod g, s = 0: the coefficient of x^0 is bit position r - 1
        v[(code_.gdeg - 1) >> 5] = 0x80000000u >> ((code_.gdeg - 1) & 31);
        long long s = 0;
        for (int lv = 0; lv < kEncBchLevels; lv++) {
            const long long want = 8LL * bch_seg_ << lv;
            for (; s < want; s++) ring.shift_in(v, 0);
            Rem row = v; // bit position p stands for x^(r-1-p): p = r - 1 first, then one more factor x per row upwards
            for (int p = code_.gdeg - 1; p >= 0; p--) {
                for (int w = 0; w < kEncRemWords; w++) join[((size_t)lv * 192 + p) * kEncRemWords + w] = row[w];
                ring.shift_in(row, 0);
            }
        }
        HIP_OK_AS("hipMalloc(&d_bch_tab_, tab.size() * 4)", alloc(&d_bch_tab_, tab.size()));
        HIP_OK(hipMemcpy(d_bch_tab_, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        HIP_OK_AS("hipMalloc(&d_bch_join_, join.size() * 4)", alloc(&d_bch_join_, join.size()));
        HIP_OK(hipMemcpy(d_bch_join_, join.data(), join.size() * 4, hipMemcpyHostToDevice));
        HIP_OK_AS("hipMalloc(&d_bch_cw_, max_frames * n / 8)", alloc(&d_bch_cw_, (size_t)max_frames_ * (code_.n / 8)));
    }
    if (has_ldpc_) {
        // the address table by residue: x = a q + b -> entry (group, a) of residue b (the (group, shift) form of ldpc_schedule.h)
        std::vector<std::vector<uint32_t>> by(q_);
        const uint16_t* p = ldpc_table_words(spec.table);
        for (int g = 0; g < spec.table->nrows; g++) {
            const int deg = *p++;
            for (int n = 0; n < deg; n++) by[p[n] % q_].push_back(((uint32_t)(360 * g) << 9) | (uint32_t)(p[n] / q_));
            p += deg;
        }
        std::vector<uint32_t> off(q_ + 1, 0), ent;
        for (int b = 0; b < q_; b++) { ent.insert(ent.end(), by[b].begin(), by[b].end()); off[b + 1] = (uint32_t)ent.size(); }
        HIP_OK_AS("hipMalloc(&d_ldpc_off_, off.size() * 4)", alloc(&d_ldpc_off_, off.size()));
        HIP_OK(hipMemcpy(d_ldpc_off_, off.data(), off.size() * 4, hipMemcpyHostToDevice));
        HIP_OK_AS("hipMalloc(&d_ldpc_ent_, ent.size() * 4)", alloc(&d_ldpc_ent_, ent.size()));
        HIP_OK(hipMemcpy(d_ldpc_ent_, ent.data(), ent.size() * 4, hipMemcpyHostToDevice));
        HIP_OK_AS("hipMalloc(&d_ldpc_cw_, max_frames * N / 8)", alloc(&d_ldpc_cw_, (size_t)max_frames_ * (N_ / 8)));
    }
    if (map_.n_mod) {
        HIP_OK_AS("hipMalloc(&d_points_, points.size() * 4)", alloc(&d_points_, map_.points.size()));
        HIP_OK(hipMemcpy(d_points_, map_.points.data(), map_.points.size() * 4, hipMemcpyHostToDevice));
    }
}

int EncoderHip::set_scramble(bool enable)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (!has_bch_) { call_err_.argument("no BCH stage: the BB scrambler is part of its load"); return -1; }
    if (enable && !d_scramble_) {
        std::vector<uint8_t> seq(code_.k / 8);
        bb_derandomise_sequence(seq.data(), (int)seq.size());
        if (alloc(&d_scramble_, seq.size()) != hipSuccess ||
            hipMemcpy(d_scramble_, seq.data(), seq.size(), hipMemcpyHostToDevice) != hipSuccess) { call_err_.device("scramble sequence upload failed"); return -1; }
    }
    scramble_ = enable;
    return 0;
}

int EncoderHip::encode_device(const uint8_t* d_in, int n_frames, uint8_t* d_bch_cw, uint8_t* d_ldpc_cw, float* d_syms, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_frames < 0 || n_frames > max_frames_) { call_err_ = { kSize, "n_frames exceeds max_frames" }; return -1; }
    if (d_bch_cw && !has_bch_) { call_err_.argument("d_bch_cw: this encoder has no BCH stage"); return -1; }
    if (d_ldpc_cw && !has_ldpc_) { call_err_.argument("d_ldpc_cw: this encoder has no LDPC stage"); return -1; }
    if (d_syms && !map_.n_mod) { call_err_.argument("d_syms: this encoder has no mapper"); return -1; }
    if (n_frames == 0) return 0;
    if (!d_in) { call_err_.argument("d_in is NULL"); return -1; }
    if (!d_bch_cw && !d_ldpc_cw && !d_syms) { call_err_.argument("no output requested"); return -1; }
    const size_t in_bytes = (size_t)n_frames * (in_bits() / 8);
    auto overlaps = [&](const void* p, size_t bytes) {
        const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)p;
        return p && a < b + bytes && b < a + in_bytes;
    };
    if (overlaps(d_bch_cw, (size_t)n_frames * (code_.n / 8)) || overlaps(d_ldpc_cw, (size_t)n_frames * (N_ / 8)) ||
        overlaps(d_syms, (size_t)n_frames * n_syms() * 8)) { call_err_.argument("d_in overlaps an output: encoding in place is not supported"); return -1; }
    const uint8_t* cur = d_in;
    if (has_bch_) {
        uint8_t* dst = d_bch_cw ? d_bch_cw : d_bch_cw_;
        EncBchArgs a;
        a.in = cur; a.cw = dst; a.scramble = scramble_ ? d_scramble_ : nullptr; a.tab = d_bch_tab_; a.join = d_bch_join_;
        a.kb = code_.k / 8; a.nb = code_.n / 8; a.seg = bch_seg_;
        hipLaunchKernelGGL(enc_bch_kernel, dim3(n_frames), dim3(kEncBchThreads), 0, stream, a);
        cur = dst;
    }
    if (has_ldpc_ && (d_ldpc_cw || d_syms)) {
        uint8_t* dst = d_ldpc_cw ? d_ldpc_cw : d_ldpc_cw_;
        EncLdpcArgs a;
        a.in = cur; a.cw = dst; a.off = d_ldpc_off_; a.ent = d_ldpc_ent_; a.kb = K_ / 8; a.nb = N_ / 8; a.q = q_;
        hipLaunchKernelGGL(enc_ldpc_kernel, dim3(n_frames), dim3(kEncLdpcThreads), 0, stream, a);
        cur = dst;
    }
    if (d_syms) {
        EncMapArgs a;
        a.cw = cur; a.syms = d_syms; a.points = reinterpret_cast<const float2*>(d_points_);
        a.n_syms = n_syms(); a.step = map_.step; a.nb = N_ / 8;
        for (int c = 0; c < 8; c++) { a.base[c] = map_.base[c]; a.shift[c] = map_.shift[c]; }
        a.total = (unsigned long long)n_frames * (unsigned long long)a.n_syms;
        const unsigned long long blocks = ((a.total + 1) / 2 + 255) / 256;
        const dim3 grid((unsigned)std::min<unsigned long long>(blocks, 1u << 20));
#define DVBS2_ENC_MAP(NMOD) case NMOD: hipLaunchKernelGGL(enc_map_kernel<NMOD>, grid, dim3(256), 0, stream, a); break
        switch (map_.n_mod) { DVBS2_ENC_MAP(2); DVBS2_ENC_MAP(3); DVBS2_ENC_MAP(4); DVBS2_ENC_MAP(5); DVBS2_ENC_MAP(6); DVBS2_ENC_MAP(8); default: break; }
#undef DVBS2_ENC_MAP
    }
    return launched("encoder kernel launch");
}

} // namespace dvbs2
