// dvbs2rx_hip_blocks.h -- host-side mirror (C++17, header only) of the reference blocks on the FEC hot
// path, implemented over the C ABI of libdvbs2_fec_hip.so. Same class names, make() argument order and
// meaning, forecast()/general_work() item accounting, getters and error behaviour as the reference:
//
//   gr::dvbs2rx::ldpc_decoder_bb        include/gnuradio/dvbs2rx/ldpc_decoder_bb.h:37-50, lib/ldpc_decoder_bb_impl.cc
//   gr::dvbs2rx::bch_decoder_bb         include/gnuradio/dvbs2rx/bch_decoder_bb.h,        lib/bch_decoder_bb_impl.cc
//   gr::dvbs2rx::xfecframe_demapper_cb  include/gnuradio/dvbs2rx/xfecframe_demapper_cb.h, lib/xfecframe_demapper_cb_impl.cc
//   gr::dvbs2rx::bbdeheader_bb          include/gnuradio/dvbs2rx/bbdeheader_bb.h,         lib/bbdeheader_bb_impl.cc
//   gr::dvbs2rx::rotator_cc             include/gnuradio/dvbs2rx/rotator_cc.h,            lib/rotator_cc_impl.cc
//   gr::dvbs2rx::symbol_sync_cc         include/gnuradio/dvbs2rx/symbol_sync_cc.h,        lib/symbol_sync_cc_impl.cc
//
// It deliberately does NOT depend on GNU Radio (absent from the build image): the classes expose the
// gr::block work-function signature with plain std::vector arguments, so that the reference's *_impl classes can
// either derive from these or forward to them (INTEGRATION.md shows the two-line patch). What GNU Radio itself
// provides (scheduler, buffers, message ports) stays in the reference; the llr_pdu hand-off is a callback here.
#pragma once
#include <cstdint>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dvbs2_fec_hip.h"

namespace dvbs2rx_hip {

// enumerations with the reference's values (dvb_config.h)
enum dvb_standard_t { STANDARD_DVBS2 = 0, STANDARD_DVBT2 };
enum dvb_framesize_t { FECFRAME_SHORT = 0, FECFRAME_NORMAL, FECFRAME_MEDIUM };
enum dvb_constellation_t { MOD_QPSK = 0, MOD_16QAM, MOD_64QAM, MOD_256QAM, MOD_8PSK, MOD_8APSK, MOD_16APSK, MOD_8_8APSK, MOD_32APSK };
enum dvb_outputmode_t { OM_CODEWORD = 0, OM_MESSAGE };
enum dvb_infomode_t { INFO_OFF = 0, INFO_ON };
typedef int dvb_code_rate_t; // use dvbs2_rate_from_name("C1_2") or the reference's enumerator value

typedef std::vector<int> gr_vector_int;
typedef std::vector<const void*> gr_vector_const_void_star;
typedef std::vector<void*> gr_vector_void_star;

inline void check(int rc)
{
    if (rc != DVBS2_OK) throw std::runtime_error(dvbs2_last_error());
}

// ---------------------------------------------------------------------------------------------- LDPC
class ldpc_decoder_bb {
public:
    typedef std::shared_ptr<ldpc_decoder_bb> sptr;
    // batch_frames replaces the reference's d_simd_size as the scheduling granule: general_work consumes whole
    // multiples of it; group_size keeps the reference's batch-coupled stopping rule (32 = AVX2, 16 otherwise).
    static sptr make(dvb_standard_t standard, dvb_framesize_t framesize, dvb_code_rate_t rate,
                     dvb_constellation_t /*constellation*/, dvb_outputmode_t outputmode, dvb_infomode_t /*infomode*/,
                     int max_trials, int /*debug_level*/ = 0, int group_size = 32, int batch_frames = 512, int device = 0)
    {
        return sptr(new ldpc_decoder_bb(standard, framesize, rate, outputmode, max_trials, group_size, batch_frames, device));
    }
    ~ldpc_decoder_bb() { dvbs2_ldpc_destroy(d_h); }

    // lib/ldpc_decoder_bb_impl.cc:380-389
    void forecast(int noutput_items, gr_vector_int& ninput_items_required) const
    {
        if (d_output_mode == OM_MESSAGE) ninput_items_required[0] = (noutput_items / (int)d_kldpc_bytes) * (int)d_nldpc;
        else ninput_items_required[0] = 8 * noutput_items;
    }
    int output_multiple() const { return (int)((d_output_mode ? d_kldpc_bytes : d_nldpc_bytes) * (unsigned)d_group); }

    // lib/ldpc_decoder_bb_impl.cc:394-455. Returns the items produced; *consumed gets consume_each()'s argument.
    int general_work(int noutput_items, gr_vector_int& /*ninput_items*/, gr_vector_const_void_star& input_items,
                     gr_vector_void_star& output_items, int* consumed)
    {
        const int8_t* in = static_cast<const int8_t*>(input_items[0]);
        unsigned char* out = static_cast<unsigned char*>(output_items[0]);
        const int trials = d_max_trials == 0 ? 25 : d_max_trials; // DEFAULT_TRIALS, :391,402
        const int output_size = (int)(d_output_mode ? d_kldpc_bytes : d_nldpc_bytes);
        int n_frames = noutput_items / output_size;
        n_frames -= n_frames % d_group;
        int done = 0;
        while (done < n_frames) {
            const int nf = std::min(n_frames - done, d_batch);
            const int ng = nf / d_group;
            d_ret.resize(ng);
            int8_t* llr_out = nullptr;
            if (d_llr_pdu) { d_soft.resize((size_t)nf * d_nldpc); llr_out = d_soft.data(); }
            check(dvbs2_ldpc_decode(d_h, in + (size_t)done * d_nldpc, nf, trials, d_output_mode, out + (size_t)done * output_size,
                                    llr_out, d_ret.data()));
            for (int g = 0; g < ng; g++) { // :411-419
                d_total_trials += d_ret[g] < 0 ? trials : trials - d_ret[g];
                if (d_llr_pdu) d_llr_pdu(d_frame_cnt, d_group, llr_out + (size_t)g * d_group * d_nldpc, (size_t)d_group * d_nldpc); // :422-429
                d_frame_cnt += d_group;
                d_batch_cnt++;
            }
            done += nf;
        }
        *consumed = n_frames * (int)d_nldpc;
        return n_frames * output_size;
    }
    unsigned int get_average_trials() const { return d_batch_cnt ? (unsigned)(d_total_trials / d_batch_cnt) : 0; } // .h:63
    // the llr_pdu message port: (frame_cnt, simd_size, decoded LLRs, count)
    void set_llr_pdu_handler(std::function<void(uint64_t, int, const int8_t*, size_t)> f) { d_llr_pdu = std::move(f); }

private:
    ldpc_decoder_bb(dvb_standard_t standard, dvb_framesize_t framesize, dvb_code_rate_t rate, dvb_outputmode_t outputmode,
                    int max_trials, int group_size, int batch_frames, int device)
        : d_output_mode(outputmode), d_max_trials(max_trials), d_group(group_size), d_batch(batch_frames - batch_frames % group_size)
    {
        if (d_batch < d_group) d_batch = d_group;
        dvbs2_fec_info_t fi;
        check(dvbs2_get_fec_info(standard, framesize, rate, &fi));
        d_kldpc = fi.ldpc_k; d_nldpc = fi.ldpc_n; d_kldpc_bytes = d_kldpc / 8; d_nldpc_bytes = d_nldpc / 8;
        check(dvbs2_ldpc_create(&d_h, standard, framesize, rate, group_size, d_batch, device));
    }
    dvbs2_ldpc_t* d_h = nullptr;
    unsigned d_nldpc = 0, d_nldpc_bytes = 0, d_kldpc = 0, d_kldpc_bytes = 0;
    int d_output_mode, d_max_trials, d_group, d_batch;
    uint64_t d_frame_cnt = 0, d_batch_cnt = 0, d_total_trials = 0;
    std::vector<int32_t> d_ret;
    std::vector<int8_t> d_soft;
    std::function<void(uint64_t, int, const int8_t*, size_t)> d_llr_pdu;
};

// ---------------------------------------------------------------------------------------------- BCH
class bch_decoder_bb {
public:
    typedef std::shared_ptr<bch_decoder_bb> sptr;
    static sptr make(dvb_standard_t standard, dvb_framesize_t framesize, dvb_code_rate_t rate, dvb_outputmode_t /*outputmode*/,
                     int /*debug_level*/ = 0, int batch_frames = 512, int device = 0)
    {
        return sptr(new bch_decoder_bb(standard, framesize, rate, batch_frames, device));
    }
    // also run the next block of the flowgraph, bbdescrambler_bb (lib/bbdescrambler_bb_impl.cc:67-82), in the same kernel
    void set_descramble(bool enable) { check(dvbs2_bch_set_descramble(d_h, enable ? 1 : 0)); }
    ~bch_decoder_bb() { dvbs2_bch_destroy(d_h); }
    void forecast(int noutput_items, gr_vector_int& req) const { req[0] = (noutput_items / d_k_bytes) * d_n_bytes; } // :78-82
    int output_multiple() const { return d_k_bytes; }
    // lib/bch_decoder_bb_impl.cc:84-117. A codeword on which the reference would have thrown (status -2) throws here too.
    int general_work(int noutput_items, gr_vector_int&, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items,
                     int* consumed)
    {
        const unsigned char* in = static_cast<const unsigned char*>(input_items[0]);
        unsigned char* out = static_cast<unsigned char*>(output_items[0]);
        const int n_codewords = noutput_items / d_k_bytes;
        int done = 0;
        while (done < n_codewords) {
            const int nf = std::min(n_codewords - done, d_batch);
            d_corr.resize(nf);
            check(dvbs2_bch_decode(d_h, in + (size_t)done * d_n_bytes, nf, out + (size_t)done * d_k_bytes, d_corr.data()));
            for (int i = 0; i < nf; i++) {
                if (d_corr[i] == -2) throw std::runtime_error("BCH decoder: the reference throws on this codeword (see dvbs2_fec_hip.h)");
                if (d_corr[i] == -1) d_frame_error_cnt++;
                d_frame_cnt++;
            }
            done += nf;
        }
        *consumed = n_codewords * d_n_bytes;
        return n_codewords * d_k_bytes;
    }
    uint64_t get_frame_count() const { return d_frame_cnt; }       // lib/bch_decoder_bb_impl.h:46
    uint64_t get_error_count() const { return d_frame_error_cnt; } // :47

private:
    bch_decoder_bb(dvb_standard_t standard, dvb_framesize_t framesize, dvb_code_rate_t rate, int batch_frames, int device) : d_batch(batch_frames)
    {
        check(dvbs2_bch_create(&d_h, standard, framesize, rate, batch_frames, device));
        int n, k, t;
        check(dvbs2_bch_params(d_h, &n, &k, &t));
        d_n_bytes = n / 8; d_k_bytes = k / 8;
    }
    dvbs2_bch_t* d_h = nullptr;
    int d_n_bytes = 0, d_k_bytes = 0, d_batch;
    uint64_t d_frame_cnt = 0, d_frame_error_cnt = 0;
    std::vector<int32_t> d_corr;
};

// ---------------------------------------------------------------------------------------------- BBFRAME de-header
class bbdeheader_bb {
public:
    typedef std::shared_ptr<bbdeheader_bb> sptr;
    static sptr make(dvb_standard_t standard, dvb_framesize_t framesize, dvb_code_rate_t rate, int /*debug_level*/ = 0,
                     int batch_frames = 512, int device = 0)
    {
        return sptr(new bbdeheader_bb(standard, framesize, rate, batch_frames, device));
    }
    ~bbdeheader_bb() { dvbs2_bbdeheader_destroy(d_h); }
    int output_multiple() const { return d_max_dfl / 8; }                                            // lib/bbdeheader_bb_impl.cc:62
    void forecast(int noutput_items, gr_vector_int& req) const                                       // :70-75
    {
        req[0] = (int)std::ceil((double)noutput_items * 8 / d_max_dfl) * d_kbch_bytes;
    }
    // :144-264. ninput_items[0] bytes are available; whole BBFRAMEs are consumed, whole TS packets produced.
    int general_work(int noutput_items, gr_vector_int& ninput_items, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items,
                     int* consumed)
    {
        const unsigned char* in = static_cast<const unsigned char*>(input_items[0]);
        unsigned char* out = static_cast<unsigned char*>(output_items[0]);
        const int in_bbframes = ninput_items[0] / d_kbch_bytes;
        const int out_bbframes = (int)std::ceil((double)noutput_items * 8 / d_max_dfl);
        const int n_bbframes = std::min(in_bbframes, out_bbframes);                                  // :157-161
        int done = 0, produced = 0;
        while (done < n_bbframes) {
            const int nf = std::min(n_bbframes - done, d_batch);
            d_stage.resize((size_t)nf * d_max_out);
            int64_t n = 0;
            check(dvbs2_bbdeheader_process(d_h, in + (size_t)done * d_kbch_bytes, nf, d_stage.data(), &n));
            std::memcpy(out + produced, d_stage.data(), (size_t)n);
            produced += (int)n; done += nf;
        }
        *consumed = n_bbframes * d_kbch_bytes;
        return produced;
    }
    // lib/bbdeheader_bb_impl.h:89-93
    uint64_t get_packet_count() { return counters().packets; }
    uint64_t get_error_count() { return counters().errors; }
    uint64_t get_bbframe_count() { return counters().bbframes; }
    uint64_t get_bbframe_drop_count() { return counters().dropped; }
    uint64_t get_bbframe_gap_count() { return counters().gaps; }

private:
    bbdeheader_bb(dvb_standard_t standard, dvb_framesize_t framesize, dvb_code_rate_t rate, int batch_frames, int device) : d_batch(batch_frames)
    {
        check(dvbs2_bbdeheader_create(&d_h, standard, framesize, rate, batch_frames, device));
        check(dvbs2_bbdeheader_params(d_h, &d_kbch_bytes, &d_max_dfl, &d_max_out));
    }
    dvbs2_bbdeheader_counters_t counters() { dvbs2_bbdeheader_counters_t c; check(dvbs2_bbdeheader_counters(d_h, &c, nullptr)); return c; }
    dvbs2_bbdeheader_t* d_h = nullptr;
    int d_kbch_bytes = 0, d_max_dfl = 0, d_max_out = 0, d_batch;
    std::vector<unsigned char> d_stage;
};

// ---------------------------------------------------------------------------------------------- demapper
// constellation: MOD_QPSK and MOD_8PSK as in the reference; MOD_16APSK and MOD_32APSK (DVB-S2 rates, normal and short frames) are
// this library's own -- forecast() and output_multiple() follow n_mod 4 / 5, the refinement re-maps through the natural column order.
// make_table: the caller's table of 2^n_mod points (n_mod 2, 3, 4, 5, 6 or 8; points as (re, im) floats, entry i = label i) and column
// order (column[c] = the label bit, 0 = most significant, in column c; nullptr = natural) -- dvbs2_demap_create_table. The same
// general_work and llr_pdu refinement, which re-maps through column[]. The table is the caller's: unpinned, no S2X PL signalling.
class xfecframe_demapper_cb {
public:
    typedef std::shared_ptr<xfecframe_demapper_cb> sptr;
    static sptr make(dvb_framesize_t framesize, dvb_code_rate_t rate, dvb_constellation_t constellation, int batch_frames = 512, int device = 0)
    {
        return sptr(new xfecframe_demapper_cb(framesize, rate, constellation, batch_frames, device));
    }
    static sptr make_table(dvb_framesize_t framesize, int n_mod, const float* points, const uint8_t* column, int batch_frames = 512, int device = 0)
    {
        return sptr(new xfecframe_demapper_cb(framesize, n_mod, points, column, batch_frames, device));
    }
    ~xfecframe_demapper_cb() { dvbs2_demap_destroy(d_h); }
    void forecast(int noutput_items, gr_vector_int& req) const { req[0] = noutput_items / d_n_mod; } // :95-99
    int output_multiple() const { return d_fecframe_len; }
    // lib/xfecframe_demapper_cb_impl.cc:101-186. Until the first refined estimate arrives (set_snr / the llr_pdu
    // path of the reference), N0 comes from the pre-decoder estimate of each frame, like d_waiting_first_llr.
    int general_work(int noutput_items, gr_vector_int&, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items, int* consumed)
    {
        const float* in = static_cast<const float*>(input_items[0]); // gr_complex = 2 floats
        int8_t* out = static_cast<int8_t*>(output_items[0]);
        const int n_frames = noutput_items / d_fecframe_len;
        int done = 0;
        while (done < n_frames) {
            const int nf = std::min(n_frames - done, d_batch);
            const float* p = in + (size_t)done * d_xfecframe_len * 2;
            if (d_waiting_first_llr) {
                d_n0.resize(nf);
                check(dvbs2_demap_estimate_snr(d_h, p, nf, d_n0.data()));
                for (int i = 0; i < nf; i++) { d_snr_lin = d_n0[i]; d_n0[i] = 1.0f / d_n0[i]; } // N0 = Es / snr, Es = 1
                check(dvbs2_demap_soft(d_h, p, nf, d_n0.data(), nf, out + (size_t)done * d_fecframe_len));
            } else {
                const float n0 = 1.0f / d_snr_lin;
                check(dvbs2_demap_soft(d_h, p, nf, &n0, 1, out + (size_t)done * d_fecframe_len));
            }
            for (int i = 0; i < nf; i++) { // keep the XFECFRAMEs for the post-decoder refinement (:115-123)
                d_saved[d_pool_idx] = d_frame_cnt + i;
                std::memcpy(&d_pool[d_pool_idx * (size_t)d_xfecframe_len * 2], p + (size_t)i * d_xfecframe_len * 2, (size_t)d_xfecframe_len * 8);
                d_pool_idx = (d_pool_idx + 1) % d_saved.size();
            }
            done += nf; d_frame_cnt += nf;
        }
        *consumed = n_frames * d_xfecframe_len;
        return n_frames * d_fecframe_len;
    }
    float get_snr() const { return 10.0f * std::log10(d_snr_lin); } // lib/xfecframe_demapper_cb_impl.h:74
    // refined (post-decoder) linear SNR, the result of the reference's handle_llr_pdu() (:188-318)
    void set_snr_lin(float snr_lin) { d_snr_lin = snr_lin; d_waiting_first_llr = false; }
    // The llr_pdu message handler (lib/xfecframe_demapper_cb_impl.cc:188-318): frames starting_frame_cnt ..
    // +simd_size-1 are looked up in the pool of saved XFECFRAMEs, the per-frame refined estimates (computed on the
    // GPU in one call) are averaged and become the N0 of the frames demapped from now on. Returns the number of
    // frames that were found (the reference logs and skips the others, :260-266); a malformed PDU is dropped.
    int handle_llr_pdu(uint64_t starting_frame_cnt, int simd_size, const int8_t* llr, size_t n_llr)
    {
        if (n_llr == 0 || simd_size <= 0 || n_llr != (size_t)simd_size * d_fecframe_len) return 0; // :235-239
        std::vector<float> syms; std::vector<int8_t> ref;
        int found = 0;
        for (int i = 0; i < simd_size; i++) {
            size_t idx = d_saved.size();
            for (size_t k = 0; k < d_saved.size(); k++) if (d_saved[k] == starting_frame_cnt + i) { idx = k; break; }
            if (idx == d_saved.size()) continue;
            syms.insert(syms.end(), &d_pool[idx * (size_t)d_xfecframe_len * 2], &d_pool[(idx + 1) * (size_t)d_xfecframe_len * 2]);
            ref.insert(ref.end(), llr + (size_t)i * d_fecframe_len, llr + (size_t)(i + 1) * d_fecframe_len);
            found++;
        }
        float accum = 0;
        std::vector<float> snr(d_batch);
        for (int done = 0; done < found; done += d_batch) {
            const int nf = std::min(found - done, d_batch);
            check(dvbs2_demap_refine_snr(d_h, &syms[(size_t)done * d_xfecframe_len * 2], &ref[(size_t)done * d_fecframe_len], nf, snr.data()));
            for (int i = 0; i < nf; i++) accum += snr[i];
        }
        if (found > 0) { d_snr_lin = accum / found; d_waiting_first_llr = false; } // :309-317
        return found;
    }

private:
    xfecframe_demapper_cb(dvb_framesize_t framesize, dvb_code_rate_t rate, dvb_constellation_t constellation, int batch_frames, int device) : d_batch(batch_frames)
    {
        check(dvbs2_demap_create(&d_h, framesize, rate, constellation, batch_frames, device)); // throws "Unsupported constellation" (or a rate / frame size message for 16APSK / 32APSK)
        init_pool(batch_frames);
    }
    xfecframe_demapper_cb(dvb_framesize_t framesize, int n_mod, const float* points, const uint8_t* column, int batch_frames, int device) : d_batch(batch_frames)
    {
        check(dvbs2_demap_create_table(&d_h, framesize, n_mod, points, column, batch_frames, device)); // throws with the text that names the refused argument
        init_pool(batch_frames);
    }
    void init_pool(int batch_frames)
    {
        int order;
        check(dvbs2_demap_params(d_h, &d_xfecframe_len, &d_fecframe_len, &d_n_mod, &order));
        d_saved.assign(std::max(64, 2 * batch_frames), std::numeric_limits<uint64_t>::max()); // XFECFRAME_POOL_SIZE, .h:28-32
        d_pool.resize(d_saved.size() * (size_t)d_xfecframe_len * 2);
    }
    dvbs2_demap_t* d_h = nullptr;
    int d_xfecframe_len = 0, d_fecframe_len = 0, d_n_mod = 0, d_batch;
    bool d_waiting_first_llr = true;
    float d_snr_lin = 1.0f;
    uint64_t d_frame_cnt = 0;
    std::vector<float> d_n0;
    std::vector<uint64_t> d_saved; // frame number held by each pool slot
    std::vector<float> d_pool;     // saved XFECFRAMEs, interleaved (re, im)
    size_t d_pool_idx = 0;
};

// ---------------------------------------------------------------------------------------------- rotator
// gr::dvbs2rx::rotator_cc (include/gnuradio/dvbs2rx/rotator_cc.h, lib/rotator_cc_impl.cc:36-128): a sync block, one output
// item per input item. The "cmd" message of :41-71 is the cmd() call here: `inc` with an optional absolute `offset`; without
// one the update is scheduled at the current item count (nitems_written(0), :61-63). Tagging of the updates (tag_inc_updates)
// stays with GNU Radio. The phase is evaluated in closed form on the device (include/dvbs2_fec_hip.h), not by gr::rotator's
// phasor recurrence.
class rotator_cc {
public:
    typedef std::shared_ptr<rotator_cc> sptr;
    static sptr make(double phase_inc = 0.0, bool /*tag_inc_updates*/ = false, int device = 0) { return sptr(new rotator_cc(phase_inc, device)); }
    ~rotator_cc() { dvbs2_rotator_destroy(d_h); }
    void set_phase_inc(double phase_inc) { check(dvbs2_rotator_set_phase_inc(d_h, phase_inc)); }                 // :36-39
    void cmd(double inc) { check(dvbs2_rotator_schedule(d_h, (int64_t)nitems_written(), inc)); }                 // :61-64, no offset key
    void cmd(double inc, uint64_t offset) { check(dvbs2_rotator_schedule(d_h, (int64_t)offset, inc)); }
    uint64_t nitems_written() const
    {
        int64_t n = 0;
        check(dvbs2_rotator_position(d_h, &n, nullptr));
        return (uint64_t)n;
    }
    int work(int noutput_items, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items)       // :73-128
    {
        check(dvbs2_rotator_rotate(d_h, static_cast<const float*>(input_items[0]), noutput_items, static_cast<float*>(output_items[0])));
        return noutput_items;
    }

private:
    rotator_cc(double phase_inc, int device) { check(dvbs2_rotator_create(&d_h, phase_inc, device)); }
    dvbs2_rotator_t* d_h = nullptr;
};

// ---------------------------------------------------------------------------------------------- AWGN channel
// The noise_source_c(GR_GAUSSIAN, sqrt(N0 * sps)) -> add_vcc pair of the transmit flowgraph (apps/dvbs2-tx:572-584) as one sync block
// of this library's own: one output item per input item, out = in + sigma * noise with the noise of item n a function of (seed,
// stream_id, n). `amplitude` is GNU Radio's, the standard deviation of the COMPLEX sample; the stage takes it per component,
// amplitude / sqrt 2. The item count runs in the block (nitems_written), the device keeps nothing. Unpinned against GNU Radio, whose
// generator is another one (include/dvbs2_fec_hip.h).
class awgn_cc {
public:
    typedef std::shared_ptr<awgn_cc> sptr;
    static sptr make(double amplitude, uint64_t seed = 0, uint64_t stream_id = 0, int max_items = 1 << 20, int device = 0)
    {
        return sptr(new awgn_cc(amplitude, seed, stream_id, max_items, device));
    }
    ~awgn_cc() { dvbs2_awgn_destroy(d_h); }
    void set_amplitude(double amplitude) { check(dvbs2_awgn_set_sigma(d_h, (float)(amplitude / std::sqrt(2.0)))); }
    void set_seed(uint64_t seed) { check(dvbs2_awgn_set_seed(d_h, seed)); }
    uint64_t nitems_written() const { return (uint64_t)d_written; }
    int work(int noutput_items, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items)
    {
        check(dvbs2_awgn_add(d_h, static_cast<const float*>(input_items[0]), noutput_items, d_stream_id, d_written, static_cast<float*>(output_items[0])));
        d_written += noutput_items;
        return noutput_items;
    }

private:
    awgn_cc(double amplitude, uint64_t seed, uint64_t stream_id, int max_items, int device) : d_stream_id(stream_id)
    {
        check(dvbs2_awgn_create(&d_h, seed, (float)(amplitude / std::sqrt(2.0)), 1, max_items, device));
    }
    dvbs2_awgn_t* d_h = nullptr;
    uint64_t d_stream_id;
    int64_t d_written = 0;
};

// ---------------------------------------------------------------------------------------------- symbol synchronizer
// gr::dvbs2rx::symbol_sync_cc (include/gnuradio/dvbs2rx/symbol_sync_cc.h, lib/symbol_sync_cc_impl.cc): a general block. GNU Radio
// hands general_work the input WITH the block's history in front; this mirror keeps the history in the handle on the device, so
// input_items[0] points at the first NEW sample and ninput_items[0] counts new samples only. Tag propagation is TPP_DONT in the
// reference (:265): general_work leaves the strobe indices of the call behind and map_tag_offsets() does the upper_bound placement
// of :471-487 on them -- call it after every general_work with the offsets of the tags in [nitems_read before the call,
// nitems_read after it), get the output offsets of the tags that found a strobe, and the rest stay pending for the next call.
class symbol_sync_cc {
public:
    typedef std::shared_ptr<symbol_sync_cc> sptr;
    static sptr make(float sps, float loop_bw, float damping_factor, float rolloff, int rrc_delay = 5, int n_subfilt = 128, int interp_method = 0,
                     int max_samples = 1 << 20, int device = 0)
    {
        return sptr(new symbol_sync_cc(sps, loop_bw, damping_factor, rolloff, rrc_delay, n_subfilt, interp_method, max_samples, device));
    }
    ~symbol_sync_cc() { dvbs2_symsync_destroy(d_h); }
    int history() const { return d_history; }
    uint64_t nitems_read() const { return d_n_read; }
    uint64_t nitems_written() const { return d_n_written; }
    int last_consumed() const { return d_last_consumed; }
    size_t pending_tags() const { return d_pending_tags.size(); }
    void forecast(int noutput_items, gr_vector_int& ninput_items_required) { ninput_items_required[0] = d_sps * noutput_items; } // :276-280, history apart
    int general_work(int noutput_items, gr_vector_int& ninput_items, gr_vector_const_void_star& input_items, gr_vector_void_star& output_items) // :426-495
    {
        d_strobe_idx.resize((size_t)std::max(noutput_items, 1));
        int k = 0, consumed = 0, status = 0;
        check(dvbs2_symsync_work(d_h, static_cast<const float*>(input_items[0]), ninput_items[0], static_cast<float*>(output_items[0]), noutput_items,
                                 d_strobe_idx.data(), nullptr, &k, &consumed, &status));
        if (status) throw std::runtime_error("symbol_sync_cc: the loop stopped (W1 or W2 not positive: the loop bandwidth is too wide)");
        d_strobe_idx.resize((size_t)k);
        d_read_before = d_n_read; d_written_before = d_n_written;
        d_n_read += (uint64_t)consumed; d_n_written += (uint64_t)k; d_last_consumed = consumed;
        return k;
    }
    // :446-488 for the last general_work: tag_offsets are absolute input offsets; returns the absolute output offsets of the tags placed
    std::vector<uint64_t> map_tag_offsets(const std::vector<uint64_t>& tag_offsets)
    {
        std::vector<uint64_t> tags(d_pending_tags), placed;
        tags.insert(tags.end(), tag_offsets.begin(), tag_offsets.end());
        d_pending_tags.clear();
        // the strobe indices of the handle are absolute and oblivious to the history, as the tag offsets are: of the reference's
        // strobe offset (history + subfilt_delay - 1 for polyphase, history otherwise, :471-473) the history term has cancelled
        const int64_t strobe_offset = d_interp_method == 0 ? d_subfilt_delay - 1 : 0;
        for (uint64_t t : tags) {
            const int64_t target = (int64_t)t + strobe_offset;
            const auto it = std::lower_bound(d_strobe_idx.begin(), d_strobe_idx.end(), target); // the first strobe index past or equal the target
            if (it != d_strobe_idx.end()) placed.push_back(d_written_before + (uint64_t)(it - d_strobe_idx.begin()));
            else d_pending_tags.push_back(t);
        }
        return placed;
    }

private:
    symbol_sync_cc(float sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp_method, int max_samples, int device)
        : d_sps((int)sps), d_interp_method(interp_method)
    {
        if ((std::ceil(sps) != sps) || (std::floor(sps) != sps) || ((int)sps % 2 != 0) || (sps < 2.0f)) throw std::runtime_error("sps has to be an even integer >= 2"); // :229-232
        if (interp_method < 0 || interp_method > 3) throw std::runtime_error("Invalid interpolation method (choose from 0 to 3)");                         // :258
        check(dvbs2_symsync_create(&d_h, d_sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, 1, max_samples, device));
        check(dvbs2_symsync_params(d_h, nullptr, &d_subfilt_delay, &d_history, nullptr, nullptr, nullptr));
    }
    dvbs2_symsync_t* d_h = nullptr;
    int d_sps, d_interp_method, d_history = 0, d_subfilt_delay = 0, d_last_consumed = 0;
    uint64_t d_n_read = 0, d_n_written = 0, d_read_before = 0, d_written_before = 0;
    std::vector<int64_t> d_strobe_idx;     // absolute basepoint indices of the last general_work
    std::vector<uint64_t> d_pending_tags;  // tags without a strobe yet
};

} // namespace dvbs2rx_hip
