// demap_hip.h -- soft constellation demapper (QPSK, 8PSK, 16APSK, 32APSK) behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
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
    int n_llr() const { return n_llr_; }
    int n_mod() const { return n_mod_; }
    int n_syms() const { return n_llr_ / n_mod_; }
    int column_order() const { return order_; }
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
    // QPSK and 8PSK only: the sweep kernels have no APSK arithmetic, such a chain runs demapper -> LLR buffer -> decoder
    bool fusable() const { return !is_apsk(); }

private:
    bool is_apsk() const { return n_mod_ >= 4; }
    ApskTable apsk_{}; // 16APSK / 32APSK: the points of this rate, handed to the kernels by value
    int n_llr_ = 0, n_mod_ = 0, order_ = 0, constellation_ = 0, max_frames_ = 0;
};

// The 2^n_mod points of 16APSK (DVBS2_MOD_16APSK) / 32APSK for a DVB-S2 code rate as interleaved (re, im), entry i = label i, Es = 1.
// Host only. false: not a DVB-S2 combination.
bool apsk_points(int constellation, int rate, float* re_im);

} // namespace dvbs2
