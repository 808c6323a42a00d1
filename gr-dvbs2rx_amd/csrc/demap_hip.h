// demap_hip.h -- soft constellation demapper (QPSK, 8PSK, 16APSK, 32APSK, or a caller's table of 4 .. 256 points) behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "demap_math.hpp"
#include "device_stage.h"

namespace dvbs2 {

class DemapperHip : public DeviceStage {
public:
    // framesize / rate / constellation: reference enums (dvb_config.h). Mirrors the constructor of
    // xfecframe_demapper_cb_impl (lib/xfecframe_demapper_cb_impl.cc:27-91): frame length by framesize,
    // QPSK or 8PSK ("Unsupported constellation" otherwise, :70-72), 8PSK column order by rate (:50-69). Beyond the reference:
    // 16APSK and 32APSK with the DVB-S2 rates of EN 302 307-1 table 9 / 10, normal and short frames (notes/apsk_demap.md).
    DemapperHip(int framesize, int rate, int constellation, int max_frames, int device);
    // A caller's table (demap_table_hip.hip, notes/demap_table.md): 2^n_mod points as (re, im), entry i = label i, n_mod in {2, 3, 4, 5, 6, 8};
    // column[c] = the label bit (0 = most significant) whose LLRs fill column c of a frame, nullptr = the natural order. The same exact
    // max-log LLR as 16APSK / 32APSK; the table is the caller's: neither scaled nor pinned against anything.
    DemapperHip(int framesize, int n_mod, const float* points_re_im, const uint8_t* column, int max_frames, int device);
    int n_llr() const { return n_llr_; }
    int n_mod() const { return n_mod_; }
    int n_syms() const { return n_llr_ / n_mod_; }
    int column_order() const { return order_; } // a table handle: 0 = natural order, -1 = another
    bool is_table() const { return table_; }
    void table(int* n_mod, float* points_re_im, uint8_t* column) const; // what a table handle was given; each nullable
    int max_frames() const { return max_frames_; }
    // DEVICE pointers. syms: n_frames * n_syms interleaved (re, im) floats; n0: n0_count (1 or n_frames) noise
    // energies N0 (the block's d_N0); llr_out: n_frames * n_llr int8, de-interleaved for 8PSK.
    int soft_device(const float* d_syms, int n_frames, const float* d_n0, int n0_count, int8_t* d_llr, hipStream_t stream);
    // pre-decoder linear SNR per frame (lib/xfecframe_demapper_cb_impl.cc:128-149): float reduction,
    // order differs from the reference's sequential / VOLK accumulation -> tolerance only.
    // d_ref_llr != nullptr: post-decoder refinement against the decoded LLRs (:246-317)
    int snr_device(const float* d_syms, const int8_t* d_ref_llr, int n_frames, float* d_snr, hipStream_t stream);
    // what an LDPC sweep kernel needs to do this demapper's work while it loads its frames (same arithmetic: demap_math.hpp)
    DemapFused fused(const float* d_syms, const float* d_n0, int n0_count) const;
    // QPSK and 8PSK only: the sweep kernels have no APSK or table arithmetic, such a chain runs demapper -> LLR buffer -> decoder
    bool fusable() const { return !table_ && !is_apsk(); }

private:
    bool is_apsk() const { return !table_ && n_mod_ >= 4; }
    void launch_table(const float* d_syms, int n_frames, const float* d_n0, int n0_count, int8_t* d_llr, hipStream_t stream);
    void launch_table_snr(const float* d_syms, const int8_t* d_ref_llr, int n_frames, float* d_snr, hipStream_t stream);
    const bool table_ = false;      // a caller's table
    bool table_as_apsk_ = false;    // ... of 16 points in natural order: demapped by demap_apsk_kernel<4> from apsk_, the faster of the two (notes/demap_table.md)
    std::vector<float> points_;     // ... as given,
    float* d_table_ = nullptr;      // ... on the device (at most 2 KB),
    uint8_t column_[8] = {};        // ... its column order,
    uint64_t cols_ = 0, pos_ = 0;   // ... and that for the kernels: byte c of cols_ = column[c], byte b of pos_ = the column of label bit b
    ApskTable apsk_{}; // 16APSK / 32APSK: the points of this rate, handed to the kernels by value
    int n_llr_ = 0, n_mod_ = 0, order_ = 0, constellation_ = 0, max_frames_ = 0;
};

// The 2^n_mod points of 16APSK (DVBS2_MOD_16APSK) / 32APSK for a DVB-S2 code rate as interleaved (re, im), entry i = label i, Es = 1.
// Host only. false: not a DVB-S2 combination.
bool apsk_points(int constellation, int rate, float* re_im);

// Whether (n_mod, points, column) is a table DemapperHip takes; *why (nullable) names the offending argument. Host only.
bool demap_table_check(int n_mod, const float* points_re_im, const uint8_t* column, std::string* why);

} // namespace dvbs2
