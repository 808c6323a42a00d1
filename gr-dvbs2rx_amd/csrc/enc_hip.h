// enc_hip.h -- the forward direction behind the C ABI (dvbs2_enc_*): BB scrambler -> systematic BCH -> systematic LDPC -> bit
// interleaver and mapper, each stage optional. Design, what was tried and the measured rates: notes/encoder.md.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "bch_hip.h"
#include "device_stage.h"
#include "fec_tables.h"

namespace dvbs2 {

// What the mapper stage of an encoder is made of; n_mod == 0: no mapper.
struct EncMapper {
    int n_mod = 0;
    int step = 1;          // codeword bit of column c, symbol j: base[c] + step * j
    int base[8] = {};
    int shift[8] = {};     // the bit of column c is bit `shift[c]` of the table index
    std::vector<float> points; // 2^n_mod (re, im), entry = table index
};

// BCH stage: bch_m == 0 absent. LDPC stage: table == nullptr absent.
struct EncSpec {
    int bch_m = 0; uint32_t bch_prim = 0; int bch_t = 0, bch_n = 0;
    const LdpcTableDesc* table = nullptr;
    EncMapper map;
};

// The verdict on a MODCOD, host only: fills *spec (mapper included for a built-in constellation) or names the argument in *why.
// constellation: a DVBS2_MOD_* value, DVBS2_ENC_NO_MAPPER, or kEncCallerTable (the mapper is the caller's: enc_table_mapper).
constexpr int kEncCallerTable = -2;
bool enc_spec(int standard, int framesize, int rate, int constellation, EncSpec* spec, std::string* why);
// The mapper of a caller's table (validated by demap_table_check) for frames of N bits.
bool enc_table_mapper(int N, int n_mod, const float* points_re_im, const uint8_t* column, EncMapper* map, std::string* why);

class EncoderHip : public DeviceStage {
public:
    EncoderHip(const EncSpec& spec, int max_frames, int device);
    int max_frames() const { return max_frames_; }
    int in_bits() const { return has_bch_ ? code_.k : K_; }
    int bch_n() const { return has_bch_ ? code_.n : 0; }
    int ldpc_n() const { return has_ldpc_ ? N_ : 0; }
    int n_syms() const { return map_.n_mod ? N_ / map_.n_mod : 0; }
    int n_mod() const { return map_.n_mod; }
    int set_scramble(bool enable);
    // DEVICE pointers, asynchronous on `stream`, no allocation. d_in: n_frames * in_bits / 8 bytes. Each output is nullable; an output
    // nobody asked for stays in the handle's own buffer between the stages. d_in may be the beginning of d_bch_cw's frame only when the
    // two frame strides agree, which they never do: overlapping input and output is refused (kArgument).
    int encode_device(const uint8_t* d_in, int n_frames, uint8_t* d_bch_cw, uint8_t* d_ldpc_cw, float* d_syms, hipStream_t stream);

private:
    bool has_bch_ = false, has_ldpc_ = false;
    BchCode code_;
    int N_ = 0, K_ = 0, q_ = 0;
    EncMapper map_;
    int max_frames_ = 0;
    // BCH: the byte-step table of the remainder register and the x^(8 L 2^j) maps that join the segment remainders (enc_hip.hip)
    uint32_t* d_bch_tab_ = nullptr;   // [6][256]
    uint32_t* d_bch_join_ = nullptr;  // [levels][192][6]
    int bch_seg_ = 0;                 // L: message bytes per thread
    uint8_t* d_scramble_ = nullptr;
    bool scramble_ = false;
    // LDPC: per residue b the (group, shift) entries
    uint32_t* d_ldpc_off_ = nullptr;  // [q + 1]
    uint32_t* d_ldpc_ent_ = nullptr;  // (360 g) << 9 | a
    // mapper
    float* d_points_ = nullptr;
    // what the stages hand each other when the caller does not take it
    uint8_t* d_bch_cw_ = nullptr;
    uint8_t* d_ldpc_cw_ = nullptr;
};

} // namespace dvbs2
