// pl_signal.cpp -- see pl_signal.h. Host code only.
#include "pl_signal.h"
#include <vector>

namespace dvbs2 {

PlsInfo pls_parse(int plsc)
{
    PlsInfo p{};
    p.plsc = plsc; p.modcod = plsc >> 2; p.short_fecframe = (plsc >> 1) & 1; p.has_pilots = plsc & 1;
    p.dummy_frame = p.modcod == 0;
    if (p.dummy_frame) p.has_pilots = 0; // a dummy frame cannot have pilots (lib/pl_signaling.cc:25-26)
    if (p.modcod >= 1 && p.modcod <= 11) p.n_mod = 2;
    else if (p.modcod >= 12 && p.modcod <= 17) p.n_mod = 3;
    else if (p.modcod >= 18 && p.modcod <= 23) p.n_mod = 4;
    else if (p.modcod >= 24 && p.modcod <= 28) p.n_mod = 5;
    else p.n_mod = 0;
    const PlFrameShape s = pl_frame_shape(plsc);
    p.n_slots = s.n_slots; p.n_pilots = s.n_pilots; p.plframe_len = s.plframe_len;
    p.payload_len = p.plframe_len - 90;
    p.xfecframe_len = p.n_slots * 90;
    return p;
}

uint64_t plsc_codeword(int plsc)
{
    static const uint32_t G[6] = { 0x55555555u, 0x33333333u, 0x0f0f0f0fu, 0x00ff00ffu, 0x0000ffffu, 0xffffffffu };
    const int i = (plsc >> 1) & 63;
    uint32_t code32 = 0;
    for (int row = 0; row < 6; row++) if (i & (0x20 >> row)) code32 ^= G[row];
    const uint32_t b = (plsc & 1) ? ~code32 : code32; // (y1 !y1 y2 !y2 ...) when b7 = 1, (y1 y1 y2 y2 ...) otherwise
    uint64_t cw = 0;
    for (int t = 0; t < 32; t++) {
        cw |= (uint64_t)((code32 >> t) & 1) << (2 * t + 1);
        cw |= (uint64_t)((b >> t) & 1) << (2 * t);
    }
    return cw;
}

void plheader_symbols(int plsc, float* syms90)
{
    const double S = 0.7071067811865476;
    const uint64_t cw = plsc_codeword(plsc) ^ kPlscScrambler;
    for (int k = 0; k < 90; k++) {
        const int bit = plheader_bit(cw, k);
        const double sg = bit ? -1.0 : 1.0;
        syms90[2 * k] = (float)((k & 1) ? -S * sg : S * sg);
        syms90[2 * k + 1] = (float)(S * sg);
    }
}

bool pls_rank_table(const uint8_t* list, int n, uint8_t rank[128])
{
    if (n == 0) { for (int i = 0; i < 128; i++) rank[i] = (uint8_t)i; return true; }
    for (int i = 0; i < 128; i++) rank[i] = 255;
    int next = 0;
    for (int i = 0; i < n; i++) {
        if (list[i] >= 128) return false;
        if (rank[list[i]] == 255) rank[list[i]] = (uint8_t)next++;
    }
    return true;
}

void pl_scrambling_rn(int gold_code, uint8_t* rn, int n)
{
    constexpr int P = (1 << 18) - 1;
    std::vector<uint8_t> x(P), y(P);
    for (int i = 0; i < 18; i++) { x[i] = i == 0; y[i] = 1; }
    for (int i = 0; i + 18 < P; i++) {
        x[i + 18] = x[i + 7] ^ x[i];
        y[i + 18] = y[i + 10] ^ y[i + 7] ^ y[i + 5] ^ y[i];
    }
    auto z = [&](long i) { i %= P; return (uint8_t)(x[(i + gold_code) % P] ^ y[i]); };
    for (int i = 0; i < n; i++) rn[i] = (uint8_t)(2 * z((long)i + 131072) + z(i));
}

void plsync_taps(float* sof25, float* plsc32)
{
    float h[180];
    plheader_symbols(0, h);
    auto tap_im = [&](int k) { // the tap is conj(conj(h_k) h_{k-1}) = h_k conj(h_{k-1}): purely imaginary, magnitude 1
        const double im = (double)h[2 * k + 1] * h[2 * k - 2] - (double)h[2 * k] * h[2 * k - 1];
        return im < 0.0 ? -1.0f : 1.0f;
    };
    for (int k = 1; k <= 25; k++) sof25[k - 1] = tap_im(k);
    for (int i = 0; i < 32; i++) plsc32[i] = tap_im(27 + 2 * i);
}

int plcoarse_weights(int full, float* w)
{
    const unsigned L = full ? 89 : 25; // lib/pl_freq_sync.cc:74-85, the same expression in double, kept as float
    for (unsigned m = 0; m < L; m++)
        w[m] = (float)(3.0 * ((2 * L + 1.0) * (2 * L + 1.0) - (2 * m + 1.0) * (2 * m + 1.0)) / (((2 * L + 1.0) * (2 * L + 1.0) - 1) * (2 * L + 1)));
    return (int)L;
}

const char* plframer_refusal(int plsc)
{
    if (plsc < 0 || plsc > 127) return "out of range (0..127)";
    const PlsInfo p = pls_parse(plsc);
    return p.n_mod == 0 && !p.dummy_frame ? "names a reserved MODCOD (29..31)" : nullptr;
}

bool plframer_layout(const uint8_t* plsc, int n_frames, PlFramerRec* rec, int64_t* in_syms, int64_t* out_syms, std::string* err)
{
    int64_t in = 0, out = 0;
    for (int f = 0; f < n_frames; f++) {
        if (const char* why = plframer_refusal(plsc[f])) {
            if (err) *err = "plsc[" + std::to_string(f) + "] " + why;
            return false;
        }
        const PlsInfo p = pls_parse(plsc[f]);
        if (rec) rec[f] = { in, out, p.n_slots, p.n_pilots, p.plsc, p.dummy_frame };
        in += p.dummy_frame ? 0 : p.xfecframe_len;
        out += p.plframe_len;
    }
    if (in_syms) *in_syms = in;
    if (out_syms) *out_syms = out;
    return true;
}

} // namespace dvbs2
