/*
 * dvbs2_fec_hip.h -- C ABI of libdvbs2_fec_hip.so: the MI355X (gfx950) DVB-S2/S2X FEC decode path
 * (soft demapper -> layered LDPC -> BCH) as a drop-in for the compute inside the reference's three
 * GNU Radio blocks. Plain pointers and sizes only; no C++ exceptions cross this boundary; every
 * object is a handle (re-entrant across block instances, unlike the reference's global per-TU
 * LdpcDecoder, lib/ldpc_decoder/ldpc_decoder_avx2.cc:21). One caller thread per handle at a time
 * (GNU Radio calls a block's general_work from exactly one thread).
 *
 * Enumerations take the integer values of the reference's include/gnuradio/dvbs2rx/dvb_config.h
 * (dvb_standard_t :15-18, dvb_code_rate_t :20-72, dvb_framesize_t :74-78, dvb_constellation_t :80-101,
 * dvb_outputmode_t :113-116), so the blocks can pass their constructor arguments through unchanged.
 *
 * All functions return DVBS2_OK (0) or a negative DVBS2_E* code; dvbs2_last_error() gives the text.
 * "_device" variants take DEVICE pointers (HBM-resident buffers) and a hipStream_t passed as void*;
 * the plain variants take HOST pointers and stage through buffers owned by the handle.
 * There is no CPU fallback: without a usable HIP device the create calls fail with DVBS2_EDEVICE.
 */
#ifndef DVBS2_FEC_HIP_H
#define DVBS2_FEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVBS2_OK 0
#define DVBS2_EINVAL (-1)   /* bad argument / unsupported (standard, framesize, rate) */
#define DVBS2_EDEVICE (-2)  /* HIP error or no device */
#define DVBS2_ESIZE (-3)    /* n_frames exceeds the handle's max_frames */

/* dvb_standard_t */
#define DVBS2_STANDARD_DVBS2 0
#define DVBS2_STANDARD_DVBT2 1
/* dvb_framesize_t */
#define DVBS2_FECFRAME_SHORT 0
#define DVBS2_FECFRAME_NORMAL 1
#define DVBS2_FECFRAME_MEDIUM 2
/* dvb_outputmode_t */
#define DVBS2_OM_CODEWORD 0
#define DVBS2_OM_MESSAGE 1
/* dvb_constellation_t (dvb_config.h:80-101: QPSK 0, 16QAM 1, 64QAM 2, 256QAM 3, 8PSK 4, 8APSK 5, 16APSK 6, 8+8APSK 7,
 * 32APSK 8, ...). The reference demapper supports the first two below (lib/xfecframe_demapper_cb_impl.cc:45-72); 16APSK
 * and 32APSK are this library's own (DVB-S2 rates only, see the soft demapper below). Values pinned against the reference
 * header by tests/test_oracle_kat.py::test_enums_match_reference and tests/test_apsk_model.py (tests/golden/dvb_config_enums.json). */
#define DVBS2_MOD_QPSK 0
#define DVBS2_MOD_8PSK 4
#define DVBS2_MOD_16APSK 6
#define DVBS2_MOD_32APSK 8

const char* dvbs2_last_error(void);
int dvbs2_device_count(void);

/* Page-lock a host buffer that the block hands to the plain (host-pointer) entry points again and again -- e.g. a GNU
 * Radio input buffer, once, at start() -- so that the transfers run at PCIe speed and asynchronously (pageable memory
 * goes through a staging copy at a fraction of it and blocks the calling thread). Optional; undo before freeing. Register whole
 * mappings of their own (an mmap'ed buffer), not pieces of the malloc heap; where the caller can choose its memory: dvbs2_host_alloc below.
 * dvbs2_ldpc_decode() also lands its results directly in bits_out / llr_out / ret when THOSE are page-locked (registered here or
 * allocated with hipHostMalloc) instead of in pinned buffers of the handle that it copies out afterwards -- the WHOLE output range has
 * to lie inside ONE registration / allocation visible to the handle's device (a range that spans two registrations with a pageable
 * hole, or any range the runtime cannot vouch for, goes through the handle's pinned buffers: slower, never wrong).
 * Device pointers handed to the *_device entry points: d_llr_in and d_llr_out are accessed with 8-byte loads / stores (align them
 * to 8 bytes: hipMalloc'ed buffers and whole-frame offsets into them are, N is a multiple of 8); a misaligned one is refused with
 * DVBS2_EINVAL. */
int dvbs2_host_register(void* p, size_t bytes);
int dvbs2_host_unregister(void* p);
/* Page-locked host memory allocated BY THE DRIVER (hipHostMalloc / hipHostFree) for callers that do not link HIP themselves: what a
 * GNU Radio >= 3.10 custom buffer allocator or a block's own staging buffer should use where it can choose. Preferred
 * over dvbs2_host_register on ordinary malloc'ed memory: a registration mirrors pages the kernel's memory management still owns
 * (transparent huge pages, compaction, fork), and round 6 saw a GPU write into registered heap memory of a long-running process fault
 * ("write access to a read-only page", Linux 6.18 with transparent_hugepage=always, intermittent); driver-allocated memory is not
 * subject to that. *p is 4096-byte aligned. (reference side: the item buffers of lib/ldpc_decoder_bb_impl.cc:394-455 / bch_decoder_bb_impl.cc:84-117) */
int dvbs2_host_alloc(void** p, size_t bytes);
int dvbs2_host_free(void* p);
/* 1 when [p, p + bytes) lies inside ONE page-locked allocation / registration as the runtime records it (the test the host-buffer
 * entry applies to the caller's buffers before it lets the copy engine address them directly), else 0. Diagnostics and tests. */
int dvbs2_host_is_page_locked(const void* p, size_t bytes);

/* ---- parameter map: replaces get_fec_info(), reference lib/fec_params.h:36-39 / fec_params.cc:16-344,
 * plus the table selection of lib/ldpc_decoder_bb_impl.cc:104-307 ---- */
typedef struct {
    uint32_t bch_k, bch_n, bch_t; /* fec_info_t::bch */
    uint32_t ldpc_k, ldpc_n;      /* fec_info_t::ldpc (ldpc_k == bch_n) */
    uint32_t table_k;             /* K of the LDPC parity table actually used */
    char table[24];               /* e.g. "S2_TABLE_B4" */
} dvbs2_fec_info_t;
int dvbs2_get_fec_info(int standard, int framesize, int rate, dvbs2_fec_info_t* out);
/* rate enumerator name ("C1_2", ...) or NULL; dvbs2_rate_from_name returns -1 when unknown */
const char* dvbs2_rate_name(int rate);
int dvbs2_rate_from_name(const char* name);

/* ---- LDPC schedule introspection (host only, no device needed): the (group, shift) entries of one
 * layer as derived from the accumulator-address table; used by the tests of the schedule compiler.
 * Returns the number of data entries of the layer (<0 on error). groups/shifts may be NULL. ---- */
int dvbs2_ldpc_table_info(const char* table, int* n, int* k, int* q, int* links_total, int* conflict_layers);
/* names of the built-in tables ("S2_TABLE_B4", "S2X_TABLE_C8", "T2_TABLE_A3", ...: the reference's DVB_*_TABLE_*
 * structs, lib/dvb_s2_tables.hh, dvb_s2x_tables.hh, dvb_t2_tables.hh) for index 0, 1, ...; NULL past the end */
const char* dvbs2_ldpc_table_name(int index);
int dvbs2_ldpc_layer_info(const char* table, int layer, int* block, int* groups, int* shifts, int max_entries);

/* ---- LDPC: replaces ldpc_*::ldpc_dec_init + ldpc_*::ldpc_dec_decode as called by
 * ldpc_decoder_bb_impl (reference lib/ldpc_decoder_bb_impl.cc:34-52, :320-347, :406-442) ----
 * group_size G = frames that share one iteration count = the reference's d_simd_size (32 with AVX2,
 * 16 otherwise, :312-345); frames [G*g, G*g+G) form group g. G = 1 decodes every frame on its own. */
typedef struct dvbs2_ldpc dvbs2_ldpc_t;
int dvbs2_ldpc_create(dvbs2_ldpc_t** h, int standard, int framesize, int rate,
                      int group_size, int max_frames, int device);
/* same, selecting a parity table by name; message_bits = bits emitted in DVBS2_OM_MESSAGE mode */
int dvbs2_ldpc_create_table(dvbs2_ldpc_t** h, const char* table, int message_bits,
                            int group_size, int max_frames, int device);
void dvbs2_ldpc_destroy(dvbs2_ldpc_t* h);
int dvbs2_ldpc_params(const dvbs2_ldpc_t* h, int* n, int* table_k, int* message_bits, int* q, int* group_size);
/*
 * llr_in       n_frames * N int8, frame-major, positive = bit 0 (the block's input stream, :407)
 * max_trials   iteration cap (> 0; the block maps 0 to 25 before calling, :391,402)
 * out_mode     DVBS2_OM_MESSAGE -> message_bits/8 bytes per frame, DVBS2_OM_CODEWORD -> N/8 (:404)
 * bits_out     hard decisions, MSB first (:432-442)
 * llr_out      NULL or n_frames * N decoded LLRs (the llr_pdu payload, :422-429)
 * ret          NULL or one int32 per group: what decode() returned for that batch -- trials left
 *              (max_trials - updates), or -1 when the cap was hit without convergence (:410-419)
 * n_frames need not be a multiple of G; a trailing partial group is a group of its own.
 * The batch-coupled stopping rule (every frame of a group runs exactly as many updates as the reference's SIMD batch, :153 of
 * lib/ldpc_decoder/layered_decoder.hh) is resolved on the device, inside the first launch for groups of up to 64 frames (the frames of a
 * group agree after every syndrome test); results do not depend on how frames are scheduled.
 */
int dvbs2_ldpc_decode(dvbs2_ldpc_t* h, const int8_t* llr_in, int n_frames, int max_trials, int out_mode,
                      uint8_t* bits_out, int8_t* llr_out, int32_t* ret);
int dvbs2_ldpc_decode_device(dvbs2_ldpc_t* h, const int8_t* d_llr_in, int n_frames, int max_trials,
                             int out_mode, uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret,
                             void* stream);
/* The same decode WITHOUT host synchronisation: everything (first pass, the device-side resolution of the batch-coupled
 * stopping rule, the output stage) is enqueued on `stream` and the call returns; dvbs2_ldpc_finish() waits for the stream
 * and completes the rare group that needed more rounds than were enqueued. Outputs are final once finish() returned
 * DVBS2_OK; one decode may be outstanding per handle. dvbs2_ldpc_decode_device == enqueue + finish. This is what lets a
 * block overlap the transfers and neighbours of batch k + 1 with the LDPC of batch k
 * (reference call site: lib/ldpc_decoder_bb_impl.cc:406-449, one blocking call per SIMD batch).
 * Two handles (own state each) on two streams, one call in flight on each, also hide the tail of a launch whose batches stop early
 * (measured: 0.89 -> 0.92 of the rate the iteration count allows; INTEGRATION.md "Double buffering"); the handles of one device share
 * what they need to share (the wave-pattern counters of the one-frame kernel builds), nothing else couples them. */
int dvbs2_ldpc_enqueue_device(dvbs2_ldpc_t* h, const int8_t* d_llr_in, int n_frames, int max_trials,
                              int out_mode, uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret,
                              void* stream);
int dvbs2_ldpc_finish(dvbs2_ldpc_t* h);
/* HIP-event timing of the dominant kernel (the layered update sweep) on its launch stream.
 * enable != 0 starts/reset accumulation; reads back total milliseconds and launch count. */
int dvbs2_ldpc_profile(dvbs2_ldpc_t* h, int enable, double* total_ms, int* launches);
/* Diagnostics. Host-driven resolution rounds since the handle was created: the group-synchronous stopping rule is resolved inside
 * the first launch; a frame that waited longer than the give-up threshold for its group makes finish() complete the group with resume
 * launches (results identical). Zero in normal operation -- tests and bench.py assert it. */
int dvbs2_ldpc_fallback_rounds(const dvbs2_ldpc_t* h);
/* Diagnostics. Plain hipMemcpyAsync rate of this box's host link, GB/s, best of two timed repetitions: `bytes` split evenly over
 * n_streams (1..16) concurrent streams, host memory kind 0 = hipHostMalloc, 1 = a mapping of its own + hipHostRegister (what dvbs2_host_register
 * does to a caller's buffer), 2 = pageable malloc. Beside the host-entry rates of bench.py (config2_host): is the link or the
 * pipeline what limits dvbs2_ldpc_decode? (reference call site that hands over host buffers: lib/ldpc_decoder_bb_impl.cc:406-449) */
int dvbs2_measure_host_copy(int device, size_t bytes, int n_streams, int kind, double* h2d_gbs, double* d2h_gbs);
/* Diagnostics. The shader clock of this device under VALU load, GHz: every SIMD runs dependent adds for ~1 ms; the s_memtime delta (what the
 * cycle stamps and the SQ cycle counters count in) over the s_memrealtime delta (100 MHz) of one workgroup. bench.py converts the SQ pass's
 * cycle counts with it instead of assuming the nominal 2.4 GHz (roofline.limiter). kernel_ms (nullable): duration of the probe. */
int dvbs2_measure_shader_clock(int device, double* ghz, double* kernel_ms);
/* Diagnostics / tests. The one-frame sweep kernels keep one array of per-CU wave-pattern counters PER DEVICE, shared by all handles of that
 * device (two workgroups on a CU take complementary patterns whichever handle launched them). Returns the array kept for `device_key`
 * (created on `device` when the key is new) and how many of its words are non-zero (all zero while no sweep kernel runs): the same key gives
 * the same array, another key another one -- exercised with keys a one-GPU box does not have (the multi-GPU split of SURVEY 8(e) runs one
 * process per GPU, but several handles on several devices of ONE process are allowed: INTEGRATION.md). */
int dvbs2_debug_cu_slot_table(int device, int device_key, unsigned long long* table_address, int* nonzero_words);
/* which sweep kernel the handle launches, as rocprofv3 names it: "ldpc_layered_kernel<DMAX>" or
 * "ldpc_layered_pr_kernel" (parity LLRs kept in registers / message records; chosen per table, identical results) */
const char* dvbs2_ldpc_kernel_name(const dvbs2_ldpc_t* h);

/* ---- BCH: replaces bch_codec<uint32_t, bitset256_t>::decode(u8_cptr_t, u8_ptr_t) as called by
 * bch_decoder_bb_impl (reference lib/bch.h:151, lib/bch_decoder_bb_impl.cc:58-66, :94-113) ----
 * The field is chosen like the block does: GF(2^16) x^16+x^5+x^3+x^2+1 for normal, GF(2^14) x^14+x^5+x^3+x+1
 * for short, GF(2^15) x^15+x^5+x^3+x^2+1 for medium frames; (n, t) from get_fec_info. */
typedef struct dvbs2_bch dvbs2_bch_t;
int dvbs2_bch_create(dvbs2_bch_t** h, int standard, int framesize, int rate, int max_frames, int device);
/* any binary BCH code over GF(2^m), 3 <= m <= 16, t <= 12, n (0 = 2^m - 1) and k multiples of 8 */
int dvbs2_bch_create_raw(dvbs2_bch_t** h, int m, uint32_t prim_poly, int t, int n, int max_frames, int device);
void dvbs2_bch_destroy(dvbs2_bch_t* h);
int dvbs2_bch_params(const dvbs2_bch_t* h, int* n, int* k, int* t);
/* generator polynomial coefficients (one byte per coefficient, index = power of x), host only;
 * returns deg g or <0. gen may be NULL. */
int dvbs2_bch_genpoly(const dvbs2_bch_t* h, uint8_t* gen, int max_coefs);
/*
 * cw           n_frames * n/8 bytes, network bit order (first bit = x^(n-1), lib/bch.cc:436-449)
 * msg          n_frames * k/8 bytes: the systematic part with the located errors flipped (lib/bch.cc:471,445-450)
 * corrections  per frame: number of corrected bits (>= 0), -1 = more than t errors / roots not all found
 *              (the block counts it in d_frame_error_cnt, lib/bch_decoder_bb_impl.cc:101-107), -2 = the
 *              reference would have thrown here (std::out_of_range from galois_field::get_exponent(0),
 *              lib/gf.h:110 via lib/bch.cc:359-367; or "Error location number out of range", lib/bch.cc:443-444)
 */
int dvbs2_bch_decode(dvbs2_bch_t* h, const uint8_t* cw, int n_frames, uint8_t* msg, int32_t* corrections);
/* Fuse the next block of the flowgraph, bbdescrambler_bb (reference lib/bbdescrambler_bb_impl.cc:67-82,
 * apps/dvbs2-rx:863-864), into the decoder's output stage: msg[j] ^= PRBS[j], j < k/8, per frame. Off by default. */
int dvbs2_bch_set_descramble(dvbs2_bch_t* h, int enable);
/* the BBFRAME energy-dispersal sequence itself (1 + x^14 + x^15, register 100101010000000, packed MSB first;
 * reference init_bb_derandomiser(), lib/bbdescrambler_bb_impl.cc:51-65), host only; n_bytes <= 8100 */
int dvbs2_bb_descramble_sequence(uint8_t* seq, int n_bytes);
/* Device pointers, asynchronous on `stream`. The handle owns the batch's syndrome words (batches of 32 frames and more compute the odd
 * syndromes of all frames as one GF(2) matrix product before the per-frame stage): calls of ONE handle must be ordered -- the same
 * stream, or synchronised by the caller --; concurrent batches take one handle each. */
int dvbs2_bch_decode_device(dvbs2_bch_t* h, const uint8_t* d_cw, int n_frames, uint8_t* d_msg,
                            int32_t* d_corrections, void* stream);

/* ---- soft demapper: replaces QpskConstellation::demap_soft (reference lib/qpsk.h:208-214) and the
 * PhaseShiftKeying<8>::soft loop + column de-interleave (lib/psk.hh:143-150,
 * lib/xfecframe_demapper_cb_impl.cc:152-176) inside xfecframe_demapper_cb_impl::general_work ----
 * constellation: DVBS2_MOD_QPSK or DVBS2_MOD_8PSK as in the reference, and beyond it DVBS2_MOD_16APSK (rates C2_3, C3_4, C4_5,
 * C5_6, C8_9, C9_10) and DVBS2_MOD_32APSK (C3_4 .. C9_10) on normal and short frames (9/10: normal only), i.e. DVB-S2 MODCODs
 * 18-28; anything else fails with DVBS2_EINVAL ("Unsupported constellation", lib/xfecframe_demapper_cb_impl.cc:70-72, or a
 * rate / frame size message). The S2X constellations (8APSK, 8+8APSK, 4+12+16rbAPSK, 64/128/256APSK) and QAM have no built-in table:
 * they go through dvbs2_demap_create_table below with the caller's table.
 * 16APSK / 32APSK: exact max-log LLRs over all points at QPSK's scale, L_b = (min_{bit b = 1} |y - s|^2 - min_{bit b = 0} |y - s|^2) / N0,
 * llr = sat8(rint(L_b)); the LLR of label bit c (0 = most significant = first interleaver column) of symbol j is byte c * n_syms + j
 * of the frame (EN 302 307-1 5.3.2 undone; column_order 0). The constellation tables are restated from EN 302 307-1 5.4.3 / 5.4.4
 * and NOT pinned against another implementation (the reference has none). */
typedef struct dvbs2_demap dvbs2_demap_t;
/* the table itself, host only (no device needed): 2 * 2^n_mod floats (re, im), entry i = the point with label i, Es = 1.
 * DVBS2_EINVAL for another constellation or a rate that DVB-S2 does not combine with it. */
int dvbs2_apsk_points(int constellation, int rate, float* re_im);
int dvbs2_demap_create(dvbs2_demap_t** h, int framesize, int rate, int constellation, int max_frames, int device);
void dvbs2_demap_destroy(dvbs2_demap_t* h);
/* A demapper for the CALLER's constellation table of 4 .. 256 labelled points: the same exact max-log LLR as 16APSK / 32APSK above, over
 * all 2^n_mod points, L_b = (min_{bit b = 1} |y - s|^2 - min_{bit b = 0} |y - s|^2) / N0, llr = sat8(rint(L_b)) (notes/demap_table.md).
 * n_mod          one of 2, 3, 4, 5, 6, 8. 7 is refused: no DVB frame length (16200, 32400, 64800) is a multiple of 7.
 * points_re_im   2 * 2^n_mod floats (re, im); entry i is the point with label i. Used as given: not scaled, Es = 1 is not required
 *                (N0 is in the table's units). Every value must be finite. The table is the caller's and is NOT pinned against anything.
 * column         n_mod bytes, a permutation of 0 .. n_mod-1: column[c] is the label bit (0 = most significant) whose LLRs fill column c
 *                of a frame, i.e. byte c * n_syms + j of a frame is the LLR of label bit column[c] of symbol j. NULL: column[c] = c.
 *                Translating a standard's interleaver column pattern for a rate into this array is the caller's business.
 * n_llr follows from framesize alone (short 16200, normal 64800, medium 32400), n_syms = n_llr / n_mod.
 * A refusal is DVBS2_EINVAL with a text that names the argument; dvbs2_demap_table_check gives the same verdict without a device (host
 * only). Every entry that takes a dvbs2_demap_t* works on such a handle; dvbs2_demap_params reports column_order 0 for the natural
 * order and -1 for any other. SNR estimates: the nearest of all points before the decoder (lowest label on a tie), after it the point
 * whose label the LLR signs spell through column[]. dvbs2_demap_table reads back what the handle was given (each pointer nullable;
 * DVBS2_EINVAL on a handle of dvbs2_demap_create). S2X PL signalling is not part of this: dvbs2_plframe_* / dvbs2_plsync_* know the
 * 7-bit DVB-S2 PLSC only. */
int dvbs2_demap_table_check(int n_mod, const float* points_re_im, const uint8_t* column);
int dvbs2_demap_create_table(dvbs2_demap_t** h, int framesize, int n_mod, const float* points_re_im,
                             const uint8_t* column, int max_frames, int device);
int dvbs2_demap_table(const dvbs2_demap_t* h, int* n_mod, float* points_re_im, uint8_t* column);
/* symbols per frame (d_xfecframe_len), LLRs per frame (d_fecframe_len), bits per symbol, 8PSK column
 * order (0 = "012", 1 = "210", 2 = "102"; a table handle: 0 = natural, -1 = another) */
int dvbs2_demap_params(const dvbs2_demap_t* h, int* n_syms, int* n_llr, int* n_mod, int* column_order);
/*
 * syms      n_frames * n_syms complex symbols as interleaved (re, im) floats (gr_complex layout)
 * n0        noise energy N0 = Es/SNR (the block's d_N0, lib/xfecframe_demapper_cb_impl.cc:146-148,313-315):
 *           n0_count == 1: one value for all frames; n0_count == n_frames: one per frame
 * llr_out   n_frames * n_llr int8 LLRs, natural bit order (8PSK: de-interleaved)
 */
int dvbs2_demap_soft(dvbs2_demap_t* h, const float* syms, int n_frames, const float* n0, int n0_count,
                     int8_t* llr_out);
int dvbs2_demap_soft_device(dvbs2_demap_t* h, const float* d_syms, int n_frames, const float* d_n0,
                            int n0_count, int8_t* d_llr_out, void* stream);
/* pre-decoder linear SNR estimate per frame (lib/xfecframe_demapper_cb_impl.cc:128-149, lib/qpsk.h:240-244).
 * Float reduction in a different order than the reference: equal within tolerance, not bit-exact. */
int dvbs2_demap_estimate_snr(dvbs2_demap_t* h, const float* syms, int n_frames, float* snr_lin);
int dvbs2_demap_estimate_snr_device(dvbs2_demap_t* h, const float* d_syms, int n_frames, float* d_snr_lin,
                                    void* stream);
/* post-decoder refinement, the per-frame body of handle_llr_pdu() (lib/xfecframe_demapper_cb_impl.cc:268-307;
 * QPSK: QpskConstellation::estimate_snr(in, ref_llrs, n) lib/qpsk.h:266-281): the reference constellation point of
 * every symbol is re-mapped from the signs of the decoded LLRs (ref_llr: n_frames * n_llr int8 in the decoder's
 * natural bit order, LLR < 0 => bit 1; 8PSK bits are taken through the column interleaver), then
 * snr = sum|ref|^2 / sum|x - ref|^2 per frame. The block averages the per-frame values of one llr_pdu and sets
 * N0 = 1 / mean (:309-315). Same tolerance note as above. */
int dvbs2_demap_refine_snr(dvbs2_demap_t* h, const float* syms, const int8_t* ref_llr, int n_frames,
                           float* snr_lin);
int dvbs2_demap_refine_snr_device(dvbs2_demap_t* h, const float* d_syms, const int8_t* d_ref_llr, int n_frames,
                                  float* d_snr_lin, void* stream);

/* ---- whole chain on the device: xfecframe_demapper_cb -> ldpc_decoder_bb (OM_MESSAGE) -> bch_decoder_bb,
 * as wired in apps/dvbs2-rx:853-863; intermediate LLRs and LDPC output stay in HBM ---- */
typedef struct dvbs2_chain dvbs2_chain_t;
int dvbs2_chain_create(dvbs2_chain_t** h, int standard, int framesize, int rate, int constellation,
                       int group_size, int max_frames, int device);
/* The chain with the demapper of a caller's table (dvbs2_demap_create_table: n_mod, points_re_im, column as there); standard, framesize
 * and rate choose the LDPC and BCH codes. Every chain entry works on it. It is never fused into the LDPC sweep kernel: it runs
 * demapper -> LLR buffer -> LDPC -> BCH. */
int dvbs2_chain_create_table(dvbs2_chain_t** h, int standard, int framesize, int rate, int n_mod,
                             const float* points_re_im, const uint8_t* column, int group_size, int max_frames, int device);
void dvbs2_chain_destroy(dvbs2_chain_t* h);
/* bytes per frame out (bch k / 8), symbols per frame in */
int dvbs2_chain_params(const dvbs2_chain_t* h, int* n_syms, int* msg_bytes);
/* The chain from LLRs (ldpc_decoder_bb -> bch_decoder_bb, apps/dvbs2-rx:857-863): for constellations without a soft demapper
 * here (the reference rejects everything but QPSK and 8PSK, lib/xfecframe_demapper_cb_impl.cc:70-72; this library adds 16APSK
 * and 32APSK) the LLRs come from elsewhere; this is BASELINE config "9/10 normal" run from int8 LLRs. */
int dvbs2_chain_create_llr(dvbs2_chain_t** h, int standard, int framesize, int rate, int group_size, int max_frames,
                           int device);
/* LLRs per frame in (N), bytes per frame out (bch k / 8), group size */
int dvbs2_chain_llr_params(const dvbs2_chain_t* h, int* n_llr, int* msg_bytes, int* group_size);
/* also apply bbdescrambler_bb in the BCH output stage (dvbs2_bch_set_descramble) */
int dvbs2_chain_set_descramble(dvbs2_chain_t* h, int enable);
/* d_msg: n_frames * bch_k/8; d_ldpc_ret (nullable): one per LDPC group; d_bch_corr (nullable -> internal): per frame */
int dvbs2_chain_decode_device(dvbs2_chain_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count,
                              int max_trials, uint8_t* d_msg, int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream);

/* d_llr: n_frames * N int8 LLRs (works on chains of either kind) */
int dvbs2_chain_decode_llr_device(dvbs2_chain_t* h, const int8_t* d_llr, int n_frames, int max_trials, uint8_t* d_msg,
                                  int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream);
/* enqueue-only variants + finish, as for the LDPC decoder: all kernels of the call go to `stream` (demapper, LDPC,
 * BCH back to back, nothing waits on the host), one call may be outstanding per handle */
int dvbs2_chain_enqueue_device(dvbs2_chain_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count,
                               int max_trials, uint8_t* d_msg, int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream);
int dvbs2_chain_enqueue_llr_device(dvbs2_chain_t* h, const int8_t* d_llr, int n_frames, int max_trials, uint8_t* d_msg,
                                   int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream);
int dvbs2_chain_finish(dvbs2_chain_t* h);
/* The fused chain from HOST buffers (the "fused entry, symbols -> message bytes" of SURVEY 8(b)): what the three blocks do with the item
 * buffers GNU Radio hands them, in one call -- xfecframe_demapper_cb_impl::general_work (reference lib/xfecframe_demapper_cb_impl.cc:101-186)
 * -> ldpc_decoder_bb_impl::general_work (lib/ldpc_decoder_bb_impl.cc:394-455) -> bch_decoder_bb_impl::general_work
 * (lib/bch_decoder_bb_impl.cc:84-117), wired as in apps/dvbs2-rx:853-863.
 * syms      n_frames * n_syms complex symbols as interleaved (re, im) floats (HOST), n0 / n0_count as for dvbs2_demap_soft (HOST)
 * msg       n_frames * bch_k/8 bytes (HOST); ldpc_ret (nullable): one int32 per LDPC group; bch_corr (nullable): one int32 per frame
 * The call is cut into chunks of whole LDPC groups over four streams (the plan of dvbs2_ldpc_decode): the input copy of chunk c + 1 and
 * the output copy of chunk c - 1 run under the kernels of chunk c. Buffers that lie inside ONE page-locked allocation / registration
 * (dvbs2_host_register, hipHostMalloc) are addressed by the copy engine directly; pageable ones go through staging (slower, never wrong).
 * An 8PSK normal frame is 172.8 KB of symbols: the host link (~57 GB/s measured) bounds this entry near 320 k frames/s. */
int dvbs2_chain_decode(dvbs2_chain_t* h, const float* syms, int n_frames, const float* n0, int n0_count, int max_trials,
                       uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr);
/* the same from int8 LLRs on the host (chains of either kind): ldpc_decoder_bb -> bch_decoder_bb */
int dvbs2_chain_decode_llr(dvbs2_chain_t* h, const int8_t* llr, int n_frames, int max_trials, uint8_t* msg, int32_t* ldpc_ret,
                           int32_t* bch_corr);
/* dvbs2_ldpc_profile / dvbs2_ldpc_kernel_name of the chain's LDPC stage (the dominant kernel) */
int dvbs2_chain_ldpc_profile(dvbs2_chain_t* h, int enable, double* total_ms, int* launches);
const char* dvbs2_chain_ldpc_kernel_name(const dvbs2_chain_t* h);
/* dvbs2_ldpc_fallback_rounds of the chain's LDPC stage: zero in normal operation */
int dvbs2_chain_ldpc_fallback_rounds(const dvbs2_chain_t* h);

/* ---- the forward direction: BBFRAME bytes -> [BB scrambler] -> systematic BCH -> systematic LDPC -> bit interleaver and mapper ->
 * XFECFRAME symbols, the exact inverse of what the chain above undoes, every result bit for bit. The reference has no counterpart
 * beyond bch_codec::encode (lib/bch.cc:158-173); its transmit application takes its FEC from gr-dtv. PL framing (PLHEADER, pilots,
 * PL scrambling) is NOT part of this: dvbs2_plframer_* below takes these symbols to PLFRAMEs. BB framing (BBHEADER, TS framing) in
 * front of it is dvbs2_bbframer_*, pulse shaping behind the PLFRAMEs is dvbs2_pulse_*: with them the transmit direction is complete.
 * input       in_bits / 8 bytes per frame, first bit = bit 7; with every stage present a BBFRAME of bch_k / 8 bytes
 * BCH cw      bch_n / 8 bytes: the message unchanged (scrambled if scrambling is on), then the remainder of m(x) x^(n-k) mod g(x), highest
 *             power first -- the layout dvbs2_bch_decode reads (lib/bch.cc:158-173, :436-449). n and k are multiples of 8 (medium
 *             frames are refused as the decoder refuses them)
 * LDPC cw     N / 8 bytes, bit i = the bit whose LLR the decoder reads at index i (what DVBS2_OM_CODEWORD emits): the K systematic bits,
 *             then the N - K parity bits of p[(x + m q) mod (N - K)] ^= information bit 360 g + m for every address x of group g, and
 *             p[r] ^= p[r - 1]
 * symbols     n_syms interleaved (re, im) floats per frame, the buffer dvbs2_chain_decode_device takes.
 *             QPSK: symbol j carries bits 2 j (I) and 2 j + 1 (Q) as +-0.70710678118654752440f, bit 0 positive.
 *             8PSK: bit b_k of symbol s is codeword bit ra_k + s (the column order dvbs2_demap_params reports for the rate); the point is
 *             the one the demapper's SNR refinement re-maps from b0 b1 b2 (lib/psk.hh:152-157).
 *             16APSK, 32APSK, a caller's table: label bit column[c] of symbol j is codeword bit c * n_syms + j; the symbol is the table
 *             entry of that label, copied bit for bit (dvbs2_apsk_points, or the caller's floats).
 * Refused with DVBS2_EINVAL and a text that names the argument: a row whose bch_n is not the LDPC table's K (the shortened / punctured
 * VL-SNR and medium rows: their pattern is not in the reference and cannot be pinned; dvbs2_enc_create_parts with the table name still
 * encodes the mother code), a 16APSK / 32APSK rate DVB-S2 does not have, a built-in constellation on a DVB-T2 row (DVBS2_ENC_NO_MAPPER
 * and a caller's table are accepted there), n_mod 7, a table dvbs2_demap_table_check refuses. ---- */
typedef struct dvbs2_enc dvbs2_enc_t;
#define DVBS2_ENC_NO_MAPPER (-1)
/* the whole chain of one MODCOD; constellation: a DVBS2_MOD_* value or DVBS2_ENC_NO_MAPPER (no symbols) */
int dvbs2_enc_create(dvbs2_enc_t** h, int standard, int framesize, int rate, int constellation, int max_frames, int device);
/* the same with the caller's constellation table: n_mod, points_re_im and column as for dvbs2_demap_create_table, by the same rules */
int dvbs2_enc_create_table(dvbs2_enc_t** h, int standard, int framesize, int rate, int n_mod, const float* points_re_im,
                           const uint8_t* column, int max_frames, int device);
/* parts, for any code the library knows. bch_m == 0: no BCH stage (else as dvbs2_bch_create_raw); ldpc_table == NULL: no LDPC stage
 * (else a name of dvbs2_ldpc_table_name). At least one stage; both: bch_n must be the table's K. There is no mapper. */
int dvbs2_enc_create_parts(dvbs2_enc_t** h, int bch_m, uint32_t bch_prim_poly, int bch_t, int bch_n, const char* ldpc_table,
                           int max_frames, int device);
void dvbs2_enc_destroy(dvbs2_enc_t* h);
/* in_bits = k of the first stage present; 0 for a stage that is absent; each nullable */
int dvbs2_enc_params(const dvbs2_enc_t* h, int* in_bits, int* bch_n, int* ldpc_n, int* n_syms, int* n_mod);
/* bbscrambler: in ^= PRBS (dvbs2_bb_descramble_sequence) before BCH, fused into the BCH stage's load. Off by default. */
int dvbs2_enc_set_scramble(dvbs2_enc_t* h, int enable);
/* host only, no device needed: the verdict dvbs2_enc_create would give (DVBS2_OK, or DVBS2_EINVAL and its text) */
int dvbs2_enc_check(int standard, int framesize, int rate, int constellation);
/* DEVICE pointers, asynchronous on `stream`: no host synchronisation, no allocation; calls on one handle are ordered by the caller (as
 * for dvbs2_bch_decode_device). Each output is nullable and then not written: the handle keeps what the next stage needs, and stages
 * behind the last requested output do not run. A requested output whose stage is absent, no output at all, and d_in overlapping an
 * output (encoding in place is not supported) are DVBS2_EINVAL; n_frames > max_frames is DVBS2_ESIZE. d_syms 16-byte aligned gets
 * 16-byte stores. */
int dvbs2_enc_encode_device(dvbs2_enc_t* h, const uint8_t* d_in, int n_frames, uint8_t* d_bch_cw, uint8_t* d_ldpc_cw,
                            float* d_syms, void* stream);
/* the same on HOST pointers, synchronous, staged through buffers of the handle */
int dvbs2_enc_encode(dvbs2_enc_t* h, const uint8_t* in, int n_frames, uint8_t* bch_cw, uint8_t* ldpc_cw, float* syms);

/* ---- PL framer: XFECFRAME symbols -> PLFRAMEs (ETSI EN 302 307-1 clauses 5.5.1 - 5.5.4), the stage dvbs2_physical_cc has in the
 * reference's transmit flowgraph (apps/dvbs2-tx:619-636; the block is gr-dtv's). The exact inverse of the payload step below with zero
 * phases: multiplying by j^Rn is a swap and a sign flip, PLHEADER symbols and pilots are constants, so every output is defined bit for
 * bit. One streaming kernel, one launch per call.
 * A handle holds a gold code and a SEQUENCE: the PLSCs of the frames of one call, in stream order (mixed MODCODs and dummy frames).
 * Frame f, with the geometry dvbs2_pls_parse reports for plsc[f], occupies plframe_len output symbols from out_offset[f]:
 *   PLHEADER  90 symbols, the floats of dvbs2_plheader_symbols(plsc[f]) unchanged; not PL-scrambled
 *   payload   payload_len symbols. Payload index k lies in pilot block k / 1476 when n_pilots > 0, k % 1476 >= 1440 and k / 1476 <
 *             n_pilots (n_pilots = (n_slots - 1) >> 4: a frame whose slot count is a multiple of 16 has NO pilot block after its last
 *             segment). Before scrambling the symbol is the pilot (S, S), S = 0.70710678118654752440f, or symbol k - 36 (k / 1476)
 *             (k without pilots) of the frame's XFECFRAME at in_offset[f].
 *   dummy     MODCOD 0: 36 slots, never pilots whatever bit 0 of the PLSC says (bit 0 still selects the header); it consumes NO input
 *             and all 3240 payload symbols are (S, S) before scrambling (clause 5.5.1)
 *   PL scrambling of the payload by Rn(k) (dvbs2_pl_scrambling_rn), k restarting at 0 in every frame: (a, b) becomes (a, b), (-b, a),
 *             (-a, -b), (b, -a) for Rn = 0, 1, 2, 3. Negation is a sign flip (0.0 becomes -0.0); no multiplication takes place.
 *   closing   closing_plsc >= 0: after the last framed frame, the 90 PLHEADER symbols of that PLSC -- the layout
 *             dvbs2_plframe_process_device reads with has_trailing_header = 1, and what dvbs2_plsync_search_device needs to report the
 *             last frame under its buffer-end rule. -1: none.
 * Input: the XFECFRAMEs of the non-dummy frames back to back in sequence order; output: the PLFRAMEs back to back. Every frame length,
 * 90, 1440 and 1476 is even, so every offset is a multiple of two symbols and, from a 16-byte-aligned base, of 16 bytes: such buffers
 * get 16-byte loads and stores, 8-byte aligned ones an 8-byte path with the same bits. A caller with several MODCODs lets each
 * dvbs2_enc_* handle write its runs of frames at in_offset of the shared input buffer (dvbs2_enc_encode_device with d_syms there).
 * Refused with DVBS2_EINVAL and a text that names the argument and the frame index: a PLSC above 127 or one with a reserved MODCOD
 * (29..31), in layout, set_sequence and closing_plsc, as dvbs2_plframe_create refuses them. gold_code 0 .. 2^18-2, max_frames 1..65535. ---- */
typedef struct dvbs2_plframer dvbs2_plframer_t;
/* host only, no device needed: in_offset[n_frames], out_offset[n_frames] and the two totals; every output nullable */
int dvbs2_plframer_layout(const uint8_t* plsc, int n_frames, int64_t* in_offset, int64_t* out_offset, int64_t* in_syms,
                          int64_t* out_syms);
/* a fresh handle has an empty sequence */
int dvbs2_plframer_create(dvbs2_plframer_t** h, int gold_code, int max_frames, int device);
void dvbs2_plframer_destroy(dvbs2_plframer_t* h);
/* configuration call, synchronous, not while work of the handle is in flight; n_frames 0..max_frames (above: DVBS2_ESIZE). A refused
 * call leaves the sequence as it was. */
int dvbs2_plframer_set_sequence(dvbs2_plframer_t* h, const uint8_t* plsc, int n_frames);
/* of the sequence; each nullable */
int dvbs2_plframer_params(const dvbs2_plframer_t* h, int* n_frames, int64_t* in_syms, int64_t* out_syms);
/* DEVICE pointers, 8-byte aligned. Frames the FIRST n_frames of the sequence (above its length: DVBS2_ESIZE) and writes exactly
 * out_offset[n_frames] symbols, plus 90 for the closing header, and nothing else. Asynchronous on `stream`, no allocation, no host
 * synchronisation. n_frames == 0 returns DVBS2_OK and writes nothing; a null buffer with n_frames > 0 is DVBS2_EINVAL, but d_xfecframes
 * may be null when the framed prefix holds dummy frames only. The buffers must not overlap. */
int dvbs2_plframer_frame_device(dvbs2_plframer_t* h, const float* d_xfecframes, int n_frames, int closing_plsc,
                                float* d_plframes, void* stream);
/* the same on HOST pointers, synchronous, staged through buffers of the handle */
int dvbs2_plframer_frame(dvbs2_plframer_t* h, const float* xfecframes, int n_frames, int closing_plsc, float* plframes);

/* ---- upstream neighbour: the PLFRAME payload step of plsync_cc_impl::handle_payload()
 * (reference lib/plsync_cc_impl.cc:644-653, :727-795): PL descrambling (lib/pl_descrambler.cc:36-105), pilot
 * block removal (:480-485) and phase de-rotation, restarted at every 16-slot segment of a coarse-corrected frame
 * from the preceding pilot block's phase estimate (:759-763). What stays in the block: frame/frequency
 * synchronisation, i.e. everything that PRODUCES the per-frame parameters below.
 * gold_code   PL scrambling code n (0 .. 2^18-2); n_slots 36..360 (lib/pl_signaling.cc:28-48)
 * payload     n_frames * payload_len complex symbols (re, im), payload_len = 90 n_slots + 36 n_pilots,
 *             n_pilots = has_pilots ? (n_slots - 1) / 16 : 0 (lib/pl_signaling.cc:51-60)
 * plheader_phase[f], phase_inc[f] = 2 pi fine_foffset (used only when coarse_corrected[f] != 0, :730-732),
 * pilot_phase[f * n_pilots + i] = pl_freq_sync::get_pilot_phase(i)
 * xfecframes  n_frames * 90 n_slots complex symbols: the input of dvbs2_demap_soft
 * The rotator is a float recurrence in the reference (VOLK); here the phase of every symbol is evaluated directly:
 * equal within 1e-4 absolute per component for unit-energy symbols, not bit-exact. */
typedef struct dvbs2_plpayload dvbs2_plpayload_t;
int dvbs2_plpayload_create(dvbs2_plpayload_t** h, int gold_code, int n_slots, int has_pilots, int max_frames, int device);
void dvbs2_plpayload_destroy(dvbs2_plpayload_t* h);
int dvbs2_plpayload_params(const dvbs2_plpayload_t* h, int* payload_len, int* xfecframe_len, int* n_pilots);
int dvbs2_plpayload_process(dvbs2_plpayload_t* h, const float* payload, int n_frames, const float* plheader_phase,
                            const float* phase_inc, const int32_t* coarse_corrected, const float* pilot_phase,
                            float* xfecframes);
int dvbs2_plpayload_process_device(dvbs2_plpayload_t* h, const float* d_payload, int n_frames,
                                   const float* d_plheader_phase, const float* d_phase_inc,
                                   const int32_t* d_coarse_corrected, const float* d_pilot_phase, float* d_xfecframes,
                                   void* stream);
/* the PL scrambling sequence Rn(i) in 0..3 (ETSI EN 302 307-1 clause 5.5.4; reference lib/pl_descrambler.cc:62-98),
 * host only; n <= 33192 */
int dvbs2_pl_scrambling_rn(int gold_code, uint8_t* rn, int n);

/* ---- PLFRAME front end (completed): everything that PRODUCES the parameters of the payload step above once frame
 * boundaries are known, and the payload step itself from whole PLFRAMEs. What stays in the block: frame synchronisation (SOF search,
 * lock state machine), the coarse frequency estimate (freq_sync::estimate_coarse, a multi-frame accumulator with feedback), the
 * open-loop PLHEADER de-rotation and the rotator control messages.
 * One handle = one gold code and one PLSC (one frame geometry, pls_info_t::parse, reference lib/pl_signaling.cc:19-61); a dummy frame
 * (MODCOD 0) has no pilots whatever bit 0 says (:25-26); the reserved MODCODs 29..31 are refused.
 * plframes    n_frames whole PLFRAMEs back to back as they lie in the frame-aligned symbol stream, plframe_len = 90 (n_slots + 1) +
 *             36 n_pilots complex symbols (re, im) each, followed -- when has_trailing_header != 0 -- by the 90 PLHEADER symbols of
 *             the frame after the batch (the pilotless estimator needs them for the last frame)
 * coarse_corrected[f]  plframe_info_t::coarse_corrected of the frame (lib/plsync_cc_impl.cc:665); coarse_foffset[f] its coarse
 *             frequency offset estimate (:610), read by pilotless handles only (nullable otherwise)
 * Per frame (one wavefront each):
 *   sof_phase       arg sum_{k<26} x_k conj(sof_k)                   freq_sync::estimate_sof_phase, lib/pl_freq_sync.cc:217-220
 *   plheader_phase  arg sum_{k<90} x_k conj(h_k), h = PLHEADER of the HANDLE's PLSC   estimate_plheader_phase, :222-226; the CCM path
 *                   of lib/plsync_cc_impl.cc:595-605, :634-636
 *   pilot_phase[f * n_pilots + i] = get_pilot_phase of block i: arg of the sum of the 36 PL-descrambled pilots at payload offset
 *                   (i + 1) 1476 - 36, minus pi/4, wrapped into [-pi, pi]   estimate_pilot_phase, :228-253, :268-273
 *   fine_foffset    pilot mode: sum_i wrap(angle_pilot[i + 1] - angle_pilot[i]) / (2 pi 1476 n_pilots), angle_pilot[0] being the phase of
 *                   the LAST 36 PLHEADER symbols (:263-266, :275-300); pilotless: wrap(plheader_phase[f + 1] - plheader_phase[f]) /
 *                   (2 pi plframe_len) when |coarse_foffset[f]| <= 1 / (2 plframe_len) (:325-343). Only for coarse-corrected frames
 *                   (lib/plsync_cc_impl.cc:665-680); otherwise fine_foffset = 0 and fine_valid = 0 (new_fine_est = false), as for the
 *                   last frame of a pilotless batch without trailing header. This is the value control_rotator_freq takes (:683-691).
 *   plsc_decoded    the frame's OWN PLSC, closed-loop path of lib/plsync_cc_impl.cc:582-590: PLHEADER times exp(-j sof_phase)
 *                   (lib/pl_freq_sync.cc:429-436), then plsc_decoder::decode (lib/pl_signaling.cc:114-167) in the mode set with
 *                   set_plsc_mode: coherent soft (default; lib/pi2_bpsk.cc:181-196, lib/reed_muller.cc:203-209), coherent hard
 *                   (lib/pi2_bpsk.cc:45-74) or differential hard (:76-179; soft is ignored when coherent = 0), hard decisions decoded by
 *                   minimum Hamming distance, first minimum in list order (lib/reed_muller.cc:128-141). A report: the caller drops frames
 *                   whose PLSC is not the handle's.
 *   set_expected_pls: the enabled-codeword list of the reference's second constructor (lib/reed_muller.cc:42-55), in the caller's order;
 *                   n = 0 enables all 128; an index >= 128 is refused. In soft mode the metrics of disabled codewords stay 0.0 and the
 *                   maximum runs over all 128 entries, as in the reference: a disabled index is returned when every enabled metric is
 *                   negative. The two setters are configuration calls: not while work of the handle is in flight.
 * xfecframes  n_frames * 90 n_slots complex symbols, bit for bit what the payload step above gives for the payload slices with
 *             plheader_phase, pilot_phase as estimated and phase_inc = (float)(2 pi fine_foffset).
 * Accuracy: the hard PLSC modes are exact (integer arithmetic) wherever the decision variables are not within rounding of zero. The soft
 * mode, the phases and the frequency offset are float sums in butterfly order with atan2f, where the reference uses VOLK kernels and GNU
 * Radio's table-driven fast_atan2f, neither of which is part of the reference tree: they are tested against a float64 model under
 * bounds derived from the float32 format, and are UNPINNED against the genuine reference.
 * Every array of the estimates structure is nullable (= not wanted): device pointers for the _device entries, host pointers otherwise. */
typedef struct dvbs2_plframe dvbs2_plframe_t;
typedef struct {
    uint8_t* plsc_decoded;   /* n_frames */
    float* sof_phase;        /* n_frames */
    float* plheader_phase;   /* n_frames */
    float* pilot_phase;      /* n_frames * n_pilots */
    float* fine_foffset;     /* n_frames */
    int32_t* fine_valid;     /* n_frames */
} dvbs2_plframe_estimates_t;
int dvbs2_plframe_create(dvbs2_plframe_t** h, int gold_code, int plsc, int max_frames, int device);
void dvbs2_plframe_destroy(dvbs2_plframe_t* h);
int dvbs2_plframe_params(const dvbs2_plframe_t* h, int* plframe_len, int* payload_len, int* xfecframe_len, int* n_slots, int* n_pilots,
                         int* n_mod);
int dvbs2_plframe_set_plsc_mode(dvbs2_plframe_t* h, int coherent, int soft);
int dvbs2_plframe_set_expected_pls(dvbs2_plframe_t* h, const uint8_t* plsc_list, int n);
/* estimates only */
int dvbs2_plframe_estimate(dvbs2_plframe_t* h, const float* plframes, int n_frames, int has_trailing_header,
                           const int32_t* coarse_corrected, const float* coarse_foffset, const dvbs2_plframe_estimates_t* est);
int dvbs2_plframe_estimate_device(dvbs2_plframe_t* h, const float* d_plframes, int n_frames, int has_trailing_header,
                                  const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                                  const dvbs2_plframe_estimates_t* d_est, void* stream);
/* estimates (est nullable) + payload step */
int dvbs2_plframe_process(dvbs2_plframe_t* h, const float* plframes, int n_frames, int has_trailing_header,
                          const int32_t* coarse_corrected, const float* coarse_foffset, float* xfecframes,
                          const dvbs2_plframe_estimates_t* est);
int dvbs2_plframe_process_device(dvbs2_plframe_t* h, const float* d_plframes, int n_frames, int has_trailing_header,
                                 const int32_t* d_coarse_corrected, const float* d_coarse_foffset, float* d_xfecframes,
                                 const dvbs2_plframe_estimates_t* d_est, void* stream);
/* host only, no device needed: the 90 expected PLHEADER symbols (re, im) of a PLSC -- SOF 0x18D2E82, RM(64,7) codeword xor
 * 0x719d83c953422dfa, pi/2 BPSK (lib/pi2_bpsk.cc:18-43, lib/pl_signaling.cc:69-73) -- and pls_info_t::parse as data */
int dvbs2_plheader_symbols(int plsc, float* syms90);
int dvbs2_pls_parse(int plsc, int* plframe_len, int* payload_len, int* xfecframe_len, int* n_slots, int* n_pilots, int* n_mod);

/* ---- PLFRAME search (the frame_sync part of plsync_cc): finds the PLFRAMEs of a RAW symbol stream, so that the entries above no
 * longer need a frame-aligned input. It restates frame_sync::step (reference lib/pl_frame_sync.cc:66-243) as three kernels:
 *   metric   for EVERY symbol index n: d[n] = conj(x[n]) x[n-1] (:99), S[n] = the 25 differentials at PLHEADER positions 1..25
 *            times the SOF taps, P[n] = the 32 differentials at positions 27, 29 .. 89 (the second symbol of each PLSC pair) times
 *            the PLSC taps, metric[n] = max(|S + P|, |S - P|) (:130-150). It peaks (57 for unit-energy symbols) on the LAST PLHEADER
 *            symbol and depends on x[n-89 .. n] only. The taps are +-j; dvbs2_plsync_taps returns their imaginary parts in header
 *            order, derived from the expected PLHEADER symbols of PLSC 0 (bit 0 of a PLSC flips all 32 PLSC taps, which the
 *            maximum over S +- P absorbs; no other PLSC bit changes them). The reference's folded tables (:39-52) are not copied.
 *   tracker  the state machine of :168-243 with threshold_u = 30 while searching / found and threshold_l = 25 once locked
 *            (lib/pl_frame_sync.h:160-162; dvbs2_plsync_thresholds). searching -> found on a peak; found -> locked on a peak exactly
 *            one frame length after the last one; once locked only the expected index is looked at, a miss there counts towards
 *            unlock_thresh consecutive misses (reference default 3) and the unlock_thresh-th returns to searching. Every accepted
 *            peak, and every expected peak that failed the threshold while the lock holds (an INFERRED peak, :232-242), is the last
 *            symbol of a PLHEADER: its PLSC is decoded from the 90 symbols ending there (lib/plsync_cc_impl.cc:880, :582-594) with
 *            the decoder of dvbs2_plframe_* -- closed loop, i.e. de-rotated by the SOF phase, NOT the block's open-loop path that
 *            needs the coarse frequency estimate -- and sets the frame length. set_plsc_mode / set_expected_pls as for
 *            dvbs2_plframe_*: configuration calls, not while work of the handle is in flight. With plsc_or_minus1 >= 0 nothing is
 *            decoded and every frame has that PLSC's length (the CCM/SIS path, lib/plsync_cc_impl.cc:145-159).
 *            Reserved MODCODs 29..31: pls_info_t::parse gives them the 36-slot geometry (lib/pl_signaling.cc:41-54), so
 *            set_frame_len never refuses a decoded PLSC; the tracker likewise takes dvbs2_pls_parse's plframe_len.
 *   gather   copies the reported frames that are locked and carry wanted_plsc, in stream order, into back-to-back PLFRAMEs followed
 *            by the 90 symbols after the last of them: the layout dvbs2_plframe_process_device reads with has_trailing_header = 1.
 *            When other frames lie between two gathered ones, the "next header" a pilotless front end sees is not the adjacent one.
 * syms       n_syms complex symbols (re, im), n_syms <= max_symbols; max_symbols >= 33282 + 90 (the longest PLFRAME and a PLHEADER)
 * metric     n_syms floats. dvbs2_plsync_metric_device uses the handle's history and does not advance the handle (diagnostics).
 * frames     max_frames records, written in stream order:
 *              sof_index  absolute index (symbols since create / reset) of the first PLHEADER symbol
 *              metric     the timing metric on the last PLHEADER symbol
 *              plsc       the decoded (or fixed) PLSC
 *              flags      bit 0: a real peak (not inferred); bit 1: the state was `locked` after this header
 * Buffer-end rule: a frame is reported once, when its whole PLFRAME and the 90 symbols after it lie inside the buffer. *consumed is
 * the buffer index of the first unreported frame's SOF (0 if that SOF lies before the buffer), or n_syms when none is pending; a frame
 * that finds max_frames records written is left pending in the same way. The caller presents the stream again from there, as with
 * GNU Radio's consume(). The handle carries
 * state, frame length, unlock count, absolute offset, where to resume, and the 89 symbols before the consumed point (zeros after
 * create / reset: the reference's cleared delay lines and d_last_in = 0). *state: 0 searching, 1 found, 2 locked.
 * dvbs2_plsync_search_device is asynchronous on `stream`; dvbs2_plsync_finish waits for it and returns its counts. dvbs2_plsync_gather_device
 * refers to the buffer of the LAST search; n_frames may be max_frames when the count is not known on the host yet (the device count
 * bounds it); d_plframes needs room for the selected frames + 90 symbols and should be 16-byte aligned; *d_count = frames written.
 * One defined difference: the reference selects its even / odd PLSC delay line by d_sym_cnt & 1 (:118-121) and restarts d_sym_cnt at
 * every peak (:229); after a peak accepted at an odd count outside lock its PLSC correlation is not the sliding one for the next 63
 * symbols. PLFRAME lengths are even, so lock is never affected. Outside lock, a threshold crossing within 63 symbols of an earlier
 * one accepted at an odd count can differ. When the earlier crossing was a true header the later one cannot be a frame; when it was a
 * FALSE crossing (plentiful at low Es/N0 without an AGC), a true header ending within those 63 symbols sees a corrupted PLSC
 * correlation in the reference and may be missed there, while it is detected here. The metric here is the clean sliding correlation.
 * A call that ends before the index at which a pending frame's header is to be looked at again (e.g. fewer than 90 symbols presented
 * from a pending SOF) consumes nothing and reports nothing.
 * Accuracy: the metric is a float sum in ascending header position where the reference uses VOLK's dot product: tested against a
 * float64 model under 65 * 2^-23 * sum |x_k| |x_{k-1}| over the header, UNPINNED against the genuine reference, like the plframe
 * estimates. A value is the same bits wherever its index falls in a call, so cutting a stream into calls does not change decisions. */
typedef struct dvbs2_plsync dvbs2_plsync_t;
typedef struct {
    int64_t sof_index;
    float metric;
    uint8_t plsc, flags, reserved[2];
} dvbs2_plsync_frame_t;
int dvbs2_plsync_create(dvbs2_plsync_t** h, int plsc_or_minus1, int unlock_thresh, int max_symbols, int max_frames, int device);
void dvbs2_plsync_destroy(dvbs2_plsync_t* h);
/* the handle as created: state searching, absolute offset 0, history zeros; synchronous (waits for the device) */
int dvbs2_plsync_reset(dvbs2_plsync_t* h);
int dvbs2_plsync_set_plsc_mode(dvbs2_plsync_t* h, int coherent, int soft);
int dvbs2_plsync_set_expected_pls(dvbs2_plsync_t* h, const uint8_t* plsc_list, int n);
int dvbs2_plsync_metric_device(dvbs2_plsync_t* h, const float* d_syms, int n_syms, float* d_metric, void* stream);
int dvbs2_plsync_search_device(dvbs2_plsync_t* h, const float* d_syms, int n_syms, dvbs2_plsync_frame_t* d_frames, void* stream);
int dvbs2_plsync_finish(dvbs2_plsync_t* h, int* n_frames, int* consumed, int* state);
/* host pointers, synchronous */
int dvbs2_plsync_search(dvbs2_plsync_t* h, const float* syms, int n_syms, dvbs2_plsync_frame_t* frames, int* n_frames, int* consumed,
                        int* state);
int dvbs2_plsync_gather_device(dvbs2_plsync_t* h, const float* d_syms, const dvbs2_plsync_frame_t* d_frames, int n_frames,
                               int wanted_plsc, float* d_plframes, int32_t* d_count, void* stream);
/* host only, no device needed: imaginary parts (+-1) of the 25 SOF taps and the 32 PLSC taps in header order; the two thresholds */
int dvbs2_plsync_taps(float* sof25, float* plsc32);
int dvbs2_plsync_thresholds(float* unlocked, float* locked);

/* ---- coarse frequency offset estimate: freq_sync::estimate_coarse (reference lib/pl_freq_sync.cc:93-199) with the mode rule of
 * its caller (lib/plsync_cc_impl.cc:567-606). It PRODUCES the coarse_corrected / coarse_foffset arrays dvbs2_plframe_*_device reads.
 * Per frame: z[k] = x[k] conj(h[k]) with h the expected PLHEADER of the frame's PLSC (dvbs2_plheader_symbols; a common positive
 * scale is dropped), R[m] = sum_{k=0}^{N-m-1} z[k+m] conj(z[k]) for m = 1..L, with N = 90, L = 89 (full PLHEADER) or N = 26, L = 25
 * (SOF only), accumulated over the `period` consecutive frames of a window. On a window's last frame: theta[m] = atan2(R[m]),
 * theta[0] = 0; d[m] = theta[m+1] - theta[m] for m = 0..L-1, wrapped by one step of +-2 pi; f = clip(sum w[m] d[m] / 2 pi, +-0.5)
 * with w[m] = 3 ((2L+1)^2 - (2m+1)^2) / (((2L+1)^2 - 1)(2L+1)) (dvbs2_plcoarse_weights); coarse_corrected = |f| < 3.3875e-4; the
 * accumulator and the frame counter restart. A frame uses the full PLHEADER when the state was coarse-corrected before it, or when
 * the handle was created with a known PLSC (plsc_or_minus1 >= 0: the reference's "PLSC decoder disabled"), and the SOF otherwise; the
 * state changes on a window's last frame only, so the form is constant within a window.
 * Outputs per frame, each nullable: coarse_foffset (float: the latest estimate, 0 before the first), coarse_corrected (int32: the
 * state AFTER this frame), new_est (int32: 1 on a window's last frame). The state -- frame counter, accumulator, f, corrected flag --
 * lives on the device and carries over from call to call: a frame sequence cut into several calls (on one stream) gives the same
 * bits as one call. dvbs2_plcoarse_reset waits for the device and gives the handle as created.
 * Two ways to name the headers, both DEVICE pointers, asynchronous on `stream`:
 *   dvbs2_plcoarse_estimate_device          frame f starts at symbol f * stride_syms of d_plframes (stride_syms >= 90; the layout
 *                                           dvbs2_plsync_gather_device writes has stride = plframe_len); d_plsc: one byte per frame,
 *                                           or NULL for the handle's fixed PLSC.
 *   dvbs2_plcoarse_estimate_records_device  a raw symbol buffer and the records dvbs2_plsync_search_device left for it; base_index
 *                                           is the absolute index of d_syms[0] (0 for the first search after create / reset, then the
 *                                           sum of the `consumed` values so far), the PLSC is the record's. EVERY record is a frame
 *                                           (the reference estimates at every handled PLHEADER, locked or not). A record whose 90
 *                                           symbols do not all lie inside [0, n_syms) is passed over: it does not count towards the
 *                                           window, and its outputs repeat the state with new_est = 0.
 * dvbs2_plcoarse_estimate is the host-buffer form of the first (synchronous; it stages the 90 header symbols of each frame).
 * n_frames <= max_frames. There is no CPU fallback. dvbs2_plcoarse_weights (host only) writes the 89 (full != 0) or 25 window
 * weights as the floats the kernel uses and returns their count.
 * The message to the rotator (control_rotator_freq) is restated for a batch of streams as dvbs2_rotator_control_device in the section
 * "rotator rows" behind dvbs2_rotator_*; what stays in the GNU Radio block is the tag-delay calibration and the open-loop de-rotation
 * inside the tracker's PLSC decode.
 * Accuracy: the sums are float, each lag in ascending symbol order and the frames in order, where the reference uses VOLK's dot
 * product; the angles are atan2f where it uses gr::fast_atan2f (a table). Neither is available to compare with, so the estimate is
 * tested against a float64 model under a derived float32 bound and is UNPINNED against the genuine reference, like the plframe
 * estimates. At the three decision points -- a difference at +-pi, f at +-0.5, |f| at 3.3875e-4 -- a float evaluation may
 * legitimately decide otherwise than the model. */
typedef struct dvbs2_plcoarse dvbs2_plcoarse_t;
int dvbs2_plcoarse_create(dvbs2_plcoarse_t** h, int period, int plsc_or_minus1, int max_frames, int device);
void dvbs2_plcoarse_destroy(dvbs2_plcoarse_t* h);
int dvbs2_plcoarse_reset(dvbs2_plcoarse_t* h);
int dvbs2_plcoarse_estimate_device(dvbs2_plcoarse_t* h, const float* d_plframes, int64_t stride_syms, const uint8_t* d_plsc, int n_frames,
                                   float* d_coarse_foffset, int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream);
int dvbs2_plcoarse_estimate_records_device(dvbs2_plcoarse_t* h, const float* d_syms, int n_syms, int64_t base_index,
                                           const dvbs2_plsync_frame_t* d_frames, int n_frames, float* d_coarse_foffset,
                                           int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream);
/* host pointers, synchronous */
int dvbs2_plcoarse_estimate(dvbs2_plcoarse_t* h, const float* plframes, int64_t stride_syms, const uint8_t* plsc, int n_frames,
                            float* coarse_foffset, int32_t* coarse_corrected, int32_t* new_est);
int dvbs2_plcoarse_weights(int full, float* w);

/* ---- additive white Gaussian noise channel: the stage behind the pulse shaper of the transmit flowgraph, in front of the rotator that
 * applies the frequency offset. There (apps/dvbs2-tx:572-584) it is GNU Radio's analog.noise_source_c(GR_GAUSSIAN, sqrt(N0 * sps)) into
 * blocks.add_vcc, but GNU Radio is not in the reference tree and its generator is another one: the stage is UNPINNED against GNU Radio.
 * What is defined, and tested bit for bit against a float32 restatement (tests/awgn_model.py), is the arithmetic. The noise of complex
 * sample n (int64, >= 0) of stream s (uint64) under seed k (uint64) is a pure function of (k, s, n):
 *   words      Philox4x32-10 with counter (lo32(n >> 1), hi32(n >> 1), lo32(s), hi32(s)) and key (lo32(k), hi32(k)); sample n takes the
 *              words (w0, w1) when n is even and (w2, w3) when it is odd: wa and wb. One generator block makes two complex samples.
 *   transform  Box-Muller of u1 = (wa + 1/2) 2^-32 and u2 = (wb + 1/2) 2^-32: r = sqrt(-2 ln u1), noise = (r cos, r sin)(2 pi u2), built
 *              from integer steps, float32 polynomials and one correctly rounded float32 square root (notes/awgn.md). All 32 bits of wa
 *              count at the large end: the largest radius is sqrt(2 * 33 ln 2) = 6.76. The radius is never 0, NaN or infinite.
 *   channel    y = x + sigma * noise per component: one product, then one addition; without an input y = sigma * noise, the product alone.
 * Every operation is a single IEEE float32 operation in a written order, no fused multiply-add, denormals kept; values that are not
 * finite propagate as IEEE arithmetic says. sigma == 0 returns the input, except that a component equal to -0 comes out +0 where
 * its noise is positive (-0 + +0). sigma is the standard deviation PER COMPONENT. dvbs2_awgn_sigma (host only) gives it by the reference's
 * rule (:574-580): N0 = es / 10^(esn0_db/10), sigma = sqrt(N0 sps / 2), evaluated in double and rounded once; it refuses arguments that
 * are not finite, es <= 0 and sps < 1. dvbs2_awgn_words and dvbs2_awgn_sample (host only) are the host compilation of the same
 * arithmetic: (wa, wb) and the unit-variance noise (re, im) of one sample, which is how one frame's noise is regenerated on the CPU;
 * they refuse a negative index and a null output.
 * THERE IS NO DEVICE STATE. The handle holds the seed, the scalar sigma and the checked limits, so ANY NUMBER OF CALLS MAY BE IN FLIGHT
 * PER HANDLE -- the one difference from dvbs2_agc_* and dvbs2_pulse_* -- and however a stream is cut into calls, the bits are those
 * of one call: the caller says where a call stands. Row r of a call is stream first_stream + r (wrapping mod 2^64); it reads n_samples
 * samples at d_in + r in_stride and writes exactly n_samples at d_out + r out_stride; its sample i has the absolute index
 * first_index + i. d_in == NULL selects the noise-only form. d_sigma is nullable: n_streams floats, 4-byte aligned, one per row, which
 * replace the handle's sigma for this call and are NOT checked on the device -- a negative or non-finite entry propagates
 * arithmetically. Buffers are interleaved (re, im) floats, 8-byte aligned; strides count complex elements and matter only when
 * n_streams > 1. A lane owns one generator block, DVBS2_AWGN_TILE samples of a row to a workgroup; blocks that are 16-byte aligned in
 * every row get one 16-byte load and store, any other the 8-byte path with the same bits; a call that starts or ends on an odd absolute
 * index has a half block at that edge. d_out == d_in with equal strides is allowed and gives the bits of an out-of-place call; any other
 * overlap is not allowed and not detected. One launch per call, no allocation, no host synchronisation.
 * dvbs2_awgn_check (host only) refuses with DVBS2_EINVAL, in a text that names the argument, a sigma that is negative or not finite,
 * max_streams outside 1..65535 and max_samples outside 1..2^30; dvbs2_awgn_create applies it; dvbs2_awgn_set_sigma applies its first
 * part and, like dvbs2_awgn_set_seed, holds for the calls made after it. The add entries refuse with DVBS2_ESIZE n_samples >
 * max_samples and n_streams > max_streams, and with DVBS2_EINVAL and a text that names the argument negative counts, a negative
 * first_index or one whose last sample would pass 2^63 - 1, a null out with n_samples > 0, a misaligned buffer and, with n_streams > 1,
 * a stride below n_samples. n_samples == 0 is a successful call that does nothing. A refused call writes nothing. ---- */
typedef struct dvbs2_awgn dvbs2_awgn_t;
#define DVBS2_AWGN_TILE 512
int dvbs2_awgn_sigma(double esn0_db, double es, int sps, float* sigma);
int dvbs2_awgn_words(uint64_t seed, uint64_t stream_id, int64_t index, uint32_t* wa_wb);
int dvbs2_awgn_sample(uint64_t seed, uint64_t stream_id, int64_t index, float* re_im);
int dvbs2_awgn_check(float sigma, int max_streams, int max_samples);
int dvbs2_awgn_create(dvbs2_awgn_t** h, uint64_t seed, float sigma, int max_streams, int max_samples, int device);
void dvbs2_awgn_destroy(dvbs2_awgn_t* h);
int dvbs2_awgn_set_sigma(dvbs2_awgn_t* h, float sigma);
int dvbs2_awgn_set_seed(dvbs2_awgn_t* h, uint64_t seed);
/* each nullable */
int dvbs2_awgn_params(const dvbs2_awgn_t* h, uint64_t* seed, float* sigma, int* max_streams, int* max_samples);
/* DEVICE pointers, asynchronous on `stream`; d_in and d_sigma nullable */
int dvbs2_awgn_add_device(dvbs2_awgn_t* h, const float* d_in, int64_t in_stride, int n_samples, int n_streams, uint64_t first_stream,
                          int64_t first_index, const float* d_sigma, float* d_out, int64_t out_stride, void* stream);
/* host pointers, synchronous: one row, staged through a buffer of the handle; in nullable (noise only) */
int dvbs2_awgn_add(dvbs2_awgn_t* h, const float* in, int n_samples, uint64_t stream_id, int64_t first_index, float* out);

/* ---- IQ sample converter: the stage at the very ends of both flowgraphs, between a capture or a DAC stream of integer codes and the
 * float samples every other stage works on. In the reference's receive flowgraph (apps/dvbs2-rx:685-707) it is blocks.deinterleave,
 * uchar_to_float, add_const(-127.5), multiply_const(1/128) and float_to_complex in front of the AGC; in its transmit flowgraph
 * (apps/dvbs2-tx:533-549, apps/dvbs2-rec:439-446) complex_to_float, multiply_const(128), add_const(127.5), float_to_uchar and interleave;
 * the statistics are the block-mean form of the level reading that blocks.rms_cf gives the GUI (apps/dvbs2-rx:952). GNU Radio is not in
 * the reference tree: the stage is UNPINNED against those blocks (float_to_uchar is taken as rint plus clamp), and rms_cf itself, a
 * one-pole IIR, is not restated. What is defined, and tested bit for bit against a float32 restatement (tests/iqconv_model.py), is the
 * arithmetic (csrc/iqconv_math.hpp). One complex sample is the I code, then the Q code; with bias B, full scale F and code range [lo, hi]
 *   DVBS2_IQ_U8   B = 127.5, F = 128,   0..255            (RTL-SDR, the reference's recorder)
 *   DVBS2_IQ_S8   B = 0,     F = 128,   -128..127         (HackRF)
 *   DVBS2_IQ_S16  B = 0,     F = 32768, -32768..32767, int16 in host byte order (USRP, bladeRF, Pluto; a 12-bit device is s16, gain 16)
 *   unpack   y = (float(c) - B) / F * gain per component: the float32 nearest to that real number, one rounding ((c - B) / F is exact,
 *            and so is gain / F). With gain == 1 nothing is rounded and this is the reference's receive chain.
 *   pack     t = x * gain (one float32 product); u = t * F (exact, or infinite and then saturating); w = u + B (one float32 addition,
 *            nothing when B == 0); r = w rounded to the nearest integer, ties to even; the code is r clamped to [lo, hi]; a NaN gives
 *            the middle code, 128 for u8 and 0 for the signed formats. With gain == 1 and u8 this is the reference's transmit wiring.
 * No fused multiply-add, denormals kept. gain is a float32 of the handle, finite, positive and within [2^-64, 2^64].
 * STATISTICS are exact integers, independent of any order of summation. d_stats is nullable: n_streams x 3 uint64, 8-byte aligned; a
 * call ADDS per row {samples, clipped, energy} to it -- the caller zeroes it, and calls may be in flight concurrently on it. clipped
 * counts components: in unpack those whose code sits on a rail (lo or hi), which is how a saturated ADC reads; in pack those with
 * r < lo, r > hi or NaN -- a value that merely rounds onto the rail does not count. energy is the sum over I and Q of d * d mod 2^64,
 * d = 2 c - 255 for u8 (units of 1/256 of full scale) and d = c for the signed formats, in pack over the codes written:
 * rms = sqrt(energy / samples) / (256 or F). With d_stats == NULL the kernel does no reduction work.
 * THERE IS NO DEVICE STATE: ANY NUMBER OF DEVICE CALLS MAY BE IN FLIGHT PER HANDLE. Row r of a call reads n_samples samples at
 * d_in + r in_stride and writes exactly n_samples at d_out + r out_stride; strides count complex samples and matter only when
 * n_streams > 1. Code buffers come from files and sockets: u8 / s8 rows may start at ANY byte address, s16 rows at any even one; float
 * buffers are 8-byte aligned. Rows whose floats are 16-byte aligned and whose codes are 4-byte (s16: 8-byte) aligned in every row take
 * the wide path -- 16 bytes per lane on the float side, a dword (s16: 8 bytes) on the code side, stored whole -- and every other
 * combination a path with the same bits: an aligned interior, byte or short accesses at a row's head and tail only. Nothing outside
 * [0, n_samples) of a row is read or written. A workgroup takes DVBS2_IQCONV_TILE samples of one row. In and out have different
 * sizes: overlap is not allowed and not detected. One launch per call, no allocation, no host synchronisation.
 * dvbs2_iqconv_bytes (host only) gives the bytes of a complex sample, -1 for an unknown format. dvbs2_iqconv_check (host only) refuses
 * with DVBS2_EINVAL, in a text that names the argument, an unknown format, a gain that is not finite, not positive or outside
 * [2^-64, 2^64], max_streams outside 1..65535 and max_samples outside 1..2^30; dvbs2_iqconv_create applies it; dvbs2_iqconv_set_gain
 * applies its gain part and holds for the calls made after it. dvbs2_iqconv_unpack_host and dvbs2_iqconv_pack_host (host only) are the
 * host compilation of the same arithmetic over n samples at any host address, stats three words, nullable, ADDED to; they refuse what
 * check refuses of format and gain, a negative n and a null in or out with n > 0. The device entries refuse with DVBS2_ESIZE n_samples >
 * max_samples and n_streams > max_streams, and with DVBS2_EINVAL and a text that names the argument negative counts, a null in or out
 * with n_samples > 0, a misaligned buffer and, with n_streams > 1, a stride below n_samples. n_samples == 0 is a successful call that
 * does nothing. A refused call writes nothing and adds nothing to the statistics.
 * dvbs2_iqconv_unpack_to_device and dvbs2_iqconv_pack_from_device move HOST codes to and from DEVICE floats, one row, synchronously,
 * through a staging buffer of the handle, so that only the codes cross the host link: 2 (s16: 4) bytes per sample instead of 8. They
 * return with their output complete and the row's statistics ADDED to stats (three words on the host, nullable), and allow ONE call at
 * a time per handle. ---- */
typedef struct dvbs2_iqconv dvbs2_iqconv_t;
#define DVBS2_IQ_U8 0
#define DVBS2_IQ_S8 1
#define DVBS2_IQ_S16 2
#define DVBS2_IQCONV_TILE 8192
int dvbs2_iqconv_bytes(int format);
int dvbs2_iqconv_check(int format, float gain, int max_streams, int max_samples);
int dvbs2_iqconv_unpack_host(int format, float gain, const void* in, int64_t n, float* out, uint64_t* stats);
int dvbs2_iqconv_pack_host(int format, float gain, const float* in, int64_t n, void* out, uint64_t* stats);
int dvbs2_iqconv_create(dvbs2_iqconv_t** h, int format, float gain, int max_streams, int max_samples, int device);
void dvbs2_iqconv_destroy(dvbs2_iqconv_t* h);
int dvbs2_iqconv_set_gain(dvbs2_iqconv_t* h, float gain);
/* each nullable; tile = DVBS2_IQCONV_TILE */
int dvbs2_iqconv_params(const dvbs2_iqconv_t* h, int* format, float* gain, int* max_streams, int* max_samples, int* tile);
/* DEVICE pointers, asynchronous on `stream`; strides in complex samples; d_stats nullable */
int dvbs2_iqconv_unpack_device(dvbs2_iqconv_t* h, const void* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out,
                               int64_t out_stride, uint64_t* d_stats, void* stream);
int dvbs2_iqconv_pack_device(dvbs2_iqconv_t* h, const float* d_in, int64_t in_stride, int n_samples, int n_streams, void* d_out,
                             int64_t out_stride, uint64_t* d_stats, void* stream);
/* HOST codes <-> DEVICE floats, synchronous, one row, staged through a buffer of the handle: only the codes cross the link */
int dvbs2_iqconv_unpack_to_device(dvbs2_iqconv_t* h, const void* in, int n_samples, float* d_out, uint64_t* stats);
int dvbs2_iqconv_pack_from_device(dvbs2_iqconv_t* h, const float* d_in, int n_samples, void* out, uint64_t* stats);

/* ---- automatic gain control: the first stage of the receive flowgraph, in front of the rotator. There (apps/dvbs2-rx:873-887) it is GNU
 * Radio's analog.agc_cc(rate, reference, gain) with set_max_gain(65536) behind an optional blocks.swap_iq; the defaults are rate 1e-5,
 * reference 1, gain 1 (:1257-1269). The semantics are those of gr::analog::kernel::agc_cc::scale with max_gain, but GNU Radio is not in
 * the reference tree: the stage is UNPINNED against GNU Radio. What is defined, and tested bit for bit against a float32 restatement
 * (tests/agc_model.py), is the arithmetic. Per stream, with float32 state g and float32 parameters rate, reference, max_gain, for every
 * input sample x = (xr, xi) in order:
 *   yr = xr * g ; yi = xi * g                    (the output sample)
 *   m  = sqrt(yr*yr + yi*yi)                     two products, one addition, a correctly rounded float32 square root
 *   g  = g + rate * (reference - m)              subtraction, product, addition
 *   if (max_gain > 0 && g > max_gain) g = max_gain
 * Every operation is a single IEEE float32 operation in this order, no fused multiply-add, denormals kept. There is no lower clamp and no
 * special case for values that are not finite: a NaN or an overflow propagates exactly as IEEE arithmetic says, as in GNU Radio, and
 * dvbs2_agc_reset is the way out of a gain that is not finite. With swap_iq set, (xr, xi) is read as (xi, xr) before anything else.
 * A handle works on a batch of independent streams; each stream's gain stays on the device between calls; all streams share rate,
 * reference, max_gain and swap_iq. Stream s of a call reads n_samples samples at d_in + s in_stride and writes exactly n_samples at
 * d_out + s out_stride and -- d_gain is nullable -- one float per sample, the gain that multiplied it (g before its update), at
 * d_gain + s gain_stride. However a stream is cut into calls, the bits are those of one call. Sample buffers are interleaved (re, im)
 * floats, 8-byte aligned (d_gain: 4-byte); strides count complex elements (floats for d_gain) and matter only when n_streams > 1. Rows
 * that all start 16-byte aligned get 16-byte loads and stores, any other an 8-byte path with the same bits. d_out == d_in with equal
 * strides is allowed and gives the bits of an out-of-place call; any other overlap is not allowed and not detected. One launch per
 * call, no allocation, no host synchronisation. ONE CALL IN FLIGHT PER HANDLE, as for dvbs2_pulse_*: a call reads the gains and writes
 * them back. The kernel gives every stream a lane and walks tiles of DVBS2_AGC_TILE samples per stream (notes/agc.md).
 * dvbs2_agc_check (host only) refuses with DVBS2_EINVAL, in a text that names the argument, a rate, reference, gain or max_gain that is
 * not finite, a negative rate and a negative max_gain; max_gain == 0 means no cap, as in GNU Radio. dvbs2_agc_create applies it and
 * refuses max_streams outside 1..65535 and max_samples outside 1..2^30; dvbs2_agc_set_params applies it and holds for the calls made
 * after it, as does dvbs2_agc_set_swap_iq. dvbs2_agc_reset puts every stream's gain back to the gain of create, dvbs2_agc_set_gain sets
 * one stream's (stream_index -1: every stream's) to a finite value; both wait for the device. dvbs2_agc_state waits for the device and
 * returns the gains of streams 0 .. n_streams - 1. The work entries refuse with DVBS2_ESIZE n_samples > max_samples and n_streams >
 * max_streams, and with DVBS2_EINVAL and a text that names the argument negative counts, a null in or out with n_samples > 0, a
 * misaligned buffer and, with n_streams > 1, a stride below n_samples. n_samples == 0 is a successful call that does nothing. A refused
 * call changes no state and writes nothing. ---- */
typedef struct dvbs2_agc dvbs2_agc_t;
#define DVBS2_AGC_TILE 64
int dvbs2_agc_check(float rate, float reference, float gain, float max_gain);
int dvbs2_agc_create(dvbs2_agc_t** h, float rate, float reference, float gain, float max_gain, int max_streams, int max_samples, int device);
void dvbs2_agc_destroy(dvbs2_agc_t* h);
int dvbs2_agc_reset(dvbs2_agc_t* h);
int dvbs2_agc_set_params(dvbs2_agc_t* h, float rate, float reference, float max_gain);
int dvbs2_agc_set_swap_iq(dvbs2_agc_t* h, int enable);
int dvbs2_agc_set_gain(dvbs2_agc_t* h, int stream_index, float gain);
/* each nullable; tile = DVBS2_AGC_TILE */
int dvbs2_agc_params(const dvbs2_agc_t* h, float* rate, float* reference, float* max_gain, int* swap_iq, int* tile);
int dvbs2_agc_state(dvbs2_agc_t* h, float* gains, int n_streams);
/* DEVICE pointers, asynchronous on `stream` */
int dvbs2_agc_work_device(dvbs2_agc_t* h, const float* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out, int64_t out_stride,
                          float* d_gain, int64_t gain_stride, void* stream);
/* host pointers, synchronous: stream 0 of the handle, staged through buffers of the handle; gain nullable */
int dvbs2_agc_work(dvbs2_agc_t* h, const float* in, int n_samples, float* out, float* gain);

/* ---- rotator: rotator_cc::work (reference lib/rotator_cc_impl.cc:36-128). out[n] = in[n] e^{j phi[n]}, phi[n+1] = phi[n] + inc[n],
 * phi = 0 at the first sample after create / reset. dvbs2_rotator_set_phase_inc takes effect at once; dvbs2_rotator_schedule queues
 * an update for an ABSOLUTE sample index (counted from create / reset), across which the phase stays continuous. An update whose
 * index is already behind the handle's sample counter when a call reaches it is dropped (:92-95); one at or beyond the end of a call
 * stays queued. Updates with EQUAL indices are applied in the order they were scheduled, so the last one wins (the reference's
 * priority queue leaves that order open; this is the defined choice here). The counter is int64 and advances by n_syms per call.
 * dvbs2_rotator_seek(n) advances counter and phase over n samples exactly as calls would -- applying and dropping updates on the
 * way -- without touching data. dvbs2_rotator_reset gives the handle as created: counter 0, phase 0, the increment of create, an
 * empty queue. dvbs2_rotator_position returns the counter and the number of queued updates.
 * Buffers: complex float (re, im), 8-byte aligned; d_out == d_in is allowed, any other overlap is not. The device entry is
 * asynchronous on `stream`; schedule / set_phase_inc / seek are host-side and apply to calls made after them.
 * CLOSED FORM, not the reference's recurrence: gr::rotator multiplies a float phasor by e^{j inc} per sample and renormalises it
 * every 512 samples (volk_32fc_s32fc_x2_rotator_32fc); its error grows along the stream and one thread must walk it. Here the phase
 * is unsigned 64-bit fixed point in turns (2^64 = one turn), an increment is converted once in extended precision, the start phase
 * of every constant-increment segment is a prefix sum on the host, and sample n of a segment (n_s, P_s, I_s) has the phase
 * P_s + (n - n_s) I_s in exact integer arithmetic; its upper 32 bits go to sincospif as a float in half-turns. Hence a sample's
 * result does not depend on how the stream is cut into calls or on addresses (pieces == one call, in place == out of place, bit for
 * bit), and the phase error is at most 2^-26 + 2^-32 turns from the conversion to float plus, per sample of its segment,
 * (|inc| / 2 pi) 2^-63 + 2^-65 turns from the one rounding of the increment. VOLK is not available to compare the recurrence with:
 * the output is tested against a float64 evaluation of the exact phase under a derived bound, UNPINNED against the genuine reference. */
typedef struct dvbs2_rotator dvbs2_rotator_t;
int dvbs2_rotator_create(dvbs2_rotator_t** h, double phase_inc, int device);
void dvbs2_rotator_destroy(dvbs2_rotator_t* h);
int dvbs2_rotator_reset(dvbs2_rotator_t* h);
int dvbs2_rotator_set_phase_inc(dvbs2_rotator_t* h, double phase_inc);
int dvbs2_rotator_schedule(dvbs2_rotator_t* h, int64_t offset, double phase_inc);
int dvbs2_rotator_seek(dvbs2_rotator_t* h, int64_t n_syms);
int dvbs2_rotator_position(const dvbs2_rotator_t* h, int64_t* n_syms, int* queued);
int dvbs2_rotator_rotate_device(dvbs2_rotator_t* h, const float* d_in, int n_syms, float* d_out, void* stream);
/* host pointers, synchronous */
int dvbs2_rotator_rotate(dvbs2_rotator_t* h, const float* in, int n_syms, float* out);
/* measurement aid (tools/plcoarse_time.py): median over `regions` HIP-event regions of one rotation of n_syms symbols and, in the same
 * run, of a plain 16-byte-per-lane copy kernel over the same bytes on the same grid; it allocates 2 * 8 * n_syms bytes for the run */
int dvbs2_rotator_measure(int device, int n_syms, int regions, double* rotate_ms, double* copy_ms);

/* ---- rotator rows: the rotator for a BATCH of streams in one launch, from state held in the CALLER'S device memory, and the
 * frequency-control step that steers it from the PL estimates of one pass without a host read. There is no handle.
 * STATE. One record per stream, an array of them, 16-byte aligned, in DEVICE memory for the _device entries:
 *   phase: turns, 2^64 = one turn, AT sample `index`;  inc: turns per sample;  index: the absolute sample index `phase` refers to.
 * Sample m (absolute) of a stream has the phase  phase + (uint64_t)(m - index) * inc  modulo 2^64: exact integer arithmetic, also
 * defined for m < index. The sample itself is the single handle's (the upper 32 bits of the phase as half-turns into sincospif, four
 * products, a subtraction and an addition, no contraction): a rotated sample is a pure function of (record, absolute index), as a
 * noise sample of dvbs2_awgn_* is of (seed, stream, index). The rotation only READS the records: any number of calls may be in
 * flight, a block can be replayed, and pieces equal one call by construction. `reserved` is never read or written by a _device entry.
 * An increment changes by REBASING a record at an absolute index `at`:  phase += (at - index) * inc; index = at; inc = new.  The
 * phase stays continuous across the change: this is dvbs2_rotator_schedule(offset, inc) with the state on the device. The rotation,
 * the control step and a caller's own kernel all act on the same 32 bytes, in stream order.
 *
 * Host only, no device needed:
 *   dvbs2_rotator_state_init   phase = 0, index = 0, reserved = 0, inc = the conversion of dvbs2_rotator_create (radians per sample, in
 *                              extended precision, to 2^-64 turns, modulo one turn). A row started this way equals
 *                              dvbs2_rotator_create(phase_inc[s]) bit for bit. A phase_inc[s] that is not finite is refused, the text
 *                              names it ("phase_inc[3] must be finite"), and nothing is written. `state` is a HOST array here.
 *   dvbs2_rotator_state_read   inc and phase of HOST records back as radians in (-pi, pi]; each output nullable. For printing and tests:
 *                              a record need not be expressible in radians.
 *   dvbs2_rotator_adjust_turns the ONE conversion of the control step, so that a run can be replayed on the CPU (as dvbs2_awgn_sample
 *                              does for the noise): d = (double)estimate * scale, one float64 product; *applies = d is finite and
 *                              |d| < 0.5; *delta = d * 2^64 (exact) rounded to nearest even, which fits int64 because |d| < 0.5; without
 *                              *applies, *delta = 0.
 *   dvbs2_rotator_rows_check   the ranges dvbs2_rotator_rows_device applies first: n_streams 1..65535, n_samples 0..2^30, with
 *                              n_streams > 1 no stride below n_samples, base_index >= 0 and base_index + n_samples without overflow.
 *
 * DEVICE entries, asynchronous on `stream` (a hipStream_t) of `device`; no allocation, no host synchronisation, ONE launch each. The
 * argument checks come first, the device is looked for after them; a refused call writes nothing.
 *   dvbs2_rotator_rows_device  row s reads n_samples complex samples at d_in + 2 * s * in_stride floats and writes as many at d_out +
 *                              2 * s * out_stride; its sample i has the absolute index base_index + i, the SAME for all rows, so the
 *                              caller keeps one running int64. Buffers 8-byte aligned, strides in complex samples (they matter only with
 *                              n_streams > 1). d_out == d_in with equal strides is allowed, any other overlap is not. n_samples == 0
 *                              succeeds and launches nothing. A call does NOT split itself at a change of increment: it rotates all
 *                              its samples by the records as the device finds them; the caller cuts its calls at `at`.
 *   dvbs2_rotator_retune_device rebases record stream_index at at_index (>= 0), then inc = the conversion of phase_inc, which runs on
 *                              the host and is passed by value. stream_index is 0..65534; the array's length is the caller's to know,
 *                              as with every device array, so there is no n_streams argument and no "-1 for all".
 *   dvbs2_rotator_control_device the control rule below over the outputs of one pass: d_offsets as dvbs2_plsync_batch_gather_device
 *                              writes it (read on the DEVICE: stream s owns slots d_offsets[s] .. d_offsets[s + 1], those at or above
 *                              max_slots are ignored), the per-slot arrays of dvbs2_plcoarse_batch_estimate_device and fine_foffset /
 *                              fine_valid of dvbs2_plframe_*_strided_device. d_fine_foffset / d_fine_valid are nullable TOGETHER.
 *                              d_applied (nullable, per stream): 0 nothing, 1 a coarse step, 2 a fine step, -1 an estimate qualified but
 *                              did not apply. d_delta (nullable, per stream, int64): the turns subtracted, 0 where none were.
 * THE CONTROL RULE restates lib/plsync_cc_impl.cc:622-628 and :683-691 for a block. All slots of one pass were rotated by ONE
 * increment, so their estimates are not cumulative and the latest decides. Walking a stream's slots in order, a slot qualifies as
 * COARSE when new_est != 0 && coarse_corrected == 0, as FINE when coarse_corrected != 0 && fine_valid != 0; the LAST qualifying slot
 * of either kind decides. With its estimate e and its scale: delta = adjust_turns(e, scale); if it applies, rebase at at_index, then
 * inc -= delta (the rotator's frequency is the negative of the estimated offset). A stream without a qualifying slot is not touched
 * at all, not even rebased, and neither is one whose estimate does not apply. The reference's "locked" and "not a dummy frame"
 * conditions are met by construction: the gather copies locked frames of wanted_plsc only. The scales are gain / sps: the estimates
 * are cycles per SYMBOL and the rotator works on samples; gain is the caller's loop gain, 1 in the reference. A scale that is not
 * finite is refused on the host.
 * NOT restated: the tag-delay calibration (calibrate_tag_delay). In this block form the change takes effect at at_index, which the
 * caller sets to its running sample count: the first sample of the next call. */
typedef struct {
    uint64_t phase;
    uint64_t inc;
    int64_t index;
    uint64_t reserved;
} dvbs2_rotator_state_t;
int dvbs2_rotator_state_init(const double* phase_inc, int n_streams, dvbs2_rotator_state_t* state);
int dvbs2_rotator_state_read(const dvbs2_rotator_state_t* state, int n_streams, double* phase_inc, double* phase_at_index);
int dvbs2_rotator_adjust_turns(float estimate, double scale, int64_t* delta, int* applies);
int dvbs2_rotator_rows_check(int64_t in_stride, int64_t out_stride, int n_samples, int n_streams, int64_t base_index);
int dvbs2_rotator_rows_device(const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int n_samples, int n_streams,
                              int64_t base_index, const dvbs2_rotator_state_t* d_state, int device, void* stream);
int dvbs2_rotator_retune_device(dvbs2_rotator_state_t* d_state, int stream_index, int64_t at_index, double phase_inc, int device, void* stream);
int dvbs2_rotator_control_device(const int32_t* d_offsets, int n_streams, int max_slots, const float* d_coarse_foffset,
                                 const int32_t* d_coarse_corrected, const int32_t* d_new_est, const float* d_fine_foffset,
                                 const int32_t* d_fine_valid, double coarse_scale, double fine_scale, int64_t at_index,
                                 dvbs2_rotator_state_t* d_state, int32_t* d_applied, int64_t* d_delta, int device, void* stream);

/* ---- symbol timing recovery: symbol_sync_cc_impl::loop (reference lib/symbol_sync_cc_impl.cc:283-401) with its four interpolators
 * (:23-66, :122-132: polyphase RRC bank = the matched filter, linear, quadratic and cubic Farrow), its loop constants (:156-199), its
 * state kept across calls and the strobe indices general_work uses to move tags (:446-488). In the reference flowgraph it follows the
 * rotator and feeds plsync_cc (apps/dvbs2-rx:873-926); it takes samples at `sps` per symbol and gives symbols.
 * A call takes a BATCH of independent streams, one wavefront each (the loop is a feedback loop and cannot be cut across time): stream
 * s reads n_in[s] samples at d_in + 2 * s * in_stride floats and writes at most max_out symbols at d_out + 2 * s * out_stride floats,
 * with -- each nullable -- d_strobe_idx[s * out_stride + k] = the basepoint m_k of symbol k as an ABSOLUTE sample index of the stream
 * since create / reset, and d_mu[s * out_stride + k] = the mu used for symbol k. n_in is a HOST array. in_stride >= max n_in and
 * out_stride >= max_out when n_streams > 1. dvbs2_symsync_finish waits for the last call and returns per stream n_out, consumed and
 * status (each array nullable, n_streams entries). A handle has ONE set of per-call buffers (sample counts, results) besides the
 * per-stream state: calls on the same HIP stream may follow each other without a finish (finish then reports the last), a call on
 * another HIP stream needs dvbs2_symsync_finish first.
 * Semantics, the reference's: the history (dvbs2_symsync_geometry) starts as zeros; on a stream's first call last_xi is its first
 * sample and the loop starts at n = history + 1; the loop runs while n + jump < history + n_in and k < max_out; consumed =
 * n + 1 - history. The handle keeps, per stream and on the device, the `history` samples before the first unconsumed one and vi, cnt,
 * mu (double), jump, init, last_xi: present the stream again from `consumed`, as the GNU Radio scheduler would, and any cut of a
 * stream into calls gives the bits of one call. dvbs2_symsync_reset gives every stream as created.
 * Defined where the reference only asserts: floor(n_subfilt * mu) is clamped to 0..n_subfilt-1. A stream stops at the strobe where W1
 * or W2 is not positive (status 1) or NaN (status 2), or where the next jump is not in 1..2^30 (status 3): that strobe's symbol is
 * written and counted, n_out and consumed are reported, and later calls return at once (n_out = consumed = 0, the same status) until
 * reset; the other streams of the batch are not affected. A stream that has not started consumes nothing from a call with fewer than
 * 2 samples. Every iteration advances by at least one sample, so a call always ends.
 * Arithmetic: polyphase dot products in float, lane j of a 32-lane half summing taps j, j + 32, ... in ascending order and the halves
 * combined by a xor butterfly (16, 8, 4, 2, 1), where the reference calls VOLK; the Farrow interpolants, the Gardner error, K1 e and
 * K2 e in float in the reference's order of operations without contraction; the PI filter and the modulo-1 counter in IEEE double
 * with true divisions, as the reference. tests/symsync_model.py restates exactly this and the device is tested bit for bit against it.
 * Host only, no device needed: dvbs2_symsync_loop_constants (:156-199 with the reference's float / double mix; damping = 0 gives
 * K1 = K2 = 0, the open loop), dvbs2_symsync_geometry (history = interpolator history 1 / 3 / 3 / subfilt_len - 1 plus sps / 2;
 * subfilt_len = 2 sps rrc_delay + 1), dvbs2_symsync_taps (n_subfilt * subfilt_len floats, [subfilter][tap]: the prototype zero padded
 * to a multiple of n_subfilt, subfilter i = taps i + j n_subfilt, each subfilter flipped, :82-110). The prototype is designed from the
 * closed-form RRC impulse response with its two singular points by their limits and scaled so that the taps sum to n_subfilt
 * (firdes's convention); firdes::root_raised_cosine belongs to GNU Radio and is not available to compare with, so the bank is UNPINNED
 * against it. dvbs2_symsync_create_taps takes a caller's bank instead (firdes's own taps, laid out as above).
 * sps: an even integer 2..64; interp_method 0..3 = polyphase, linear, quadratic, cubic; rrc_delay 1..64; n_subfilt 2..4096. A bank
 * that does not fit the LDS next to the sample ring (n_subfilt * subfilt_len * 4 > 57344 bytes) or a history above 768 samples is
 * DVBS2_EINVAL. dvbs2_symsync_work is the host-buffer form for one stream (stream 0 of the handle), synchronous. */
typedef struct dvbs2_symsync dvbs2_symsync_t;
typedef struct {
    double vi, cnt, mu;
    int64_t n_read; /* samples consumed since create / reset */
    float last_xi_re, last_xi_im;
    int32_t jump, init, status, reserved;
} dvbs2_symsync_state_t;
int dvbs2_symsync_loop_constants(int sps, float loop_bw, float damping, float rolloff, float* Kp, float* K1, float* K2);
int dvbs2_symsync_geometry(int sps, int rrc_delay, int n_subfilt, int interp_method, int* subfilt_len, int* subfilt_delay, int* history);
int dvbs2_symsync_taps(int sps, float rolloff, int rrc_delay, int n_subfilt, float* bank);
int dvbs2_symsync_create(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp_method,
                         int max_streams, int max_samples, int device);
int dvbs2_symsync_create_taps(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt,
                              int interp_method, const float* bank, int max_streams, int max_samples, int device);
void dvbs2_symsync_destroy(dvbs2_symsync_t* h);
int dvbs2_symsync_reset(dvbs2_symsync_t* h);
int dvbs2_symsync_params(const dvbs2_symsync_t* h, int* subfilt_len, int* subfilt_delay, int* history, float* Kp, float* K1, float* K2);
int dvbs2_symsync_work_device(dvbs2_symsync_t* h, const float* d_in, int64_t in_stride, const int* n_in, int n_streams, float* d_out,
                              int64_t out_stride, int max_out, int64_t* d_strobe_idx, double* d_mu, void* stream);
int dvbs2_symsync_finish(dvbs2_symsync_t* h, int* n_out, int* consumed, int* status);
/* waits for the device; the state of one stream after the calls made so far */
int dvbs2_symsync_state(dvbs2_symsync_t* h, int stream_index, dvbs2_symsync_state_t* out);
/* host pointers, synchronous */
int dvbs2_symsync_work(dvbs2_symsync_t* h, const float* in, int n_in, float* out, int max_out, int64_t* strobe_idx, double* mu, int* n_out,
                       int* consumed, int* status);

/* ---- pulse shaping: PLFRAME symbols -> samples, the step behind dvbs2_plframer_* and the last one before a DAC: an integer-factor
 * interpolating FIR with real taps over complex symbols. In the reference's transmit flowgraph (apps/dvbs2-tx:638-686) it is GNU Radio's
 * interp_fir_filter_ccf over firdes.root_raised_cosine taps, optionally scaled by scale_rrc_taps (apps/dvbs2-tx:39-81). Neither block is
 * in the reference tree: the stage is UNPINNED against them (dvbs2_pulse_create_taps takes firdes's own taps). What is defined, and
 * tested bit for bit against a float32 restatement (tests/pulse_model.py), is the arithmetic:
 *   with sps samples per symbol and taps h[0 .. ntaps), sample n = m sps + p of a stream is y[n] = sum over k = 0, 1, ... while
 *   p + k sps < ntaps of h[p + k sps] * x[m - k]; real and imaginary part apart; each term a float product and then a float addition
 *   (no fused multiply-add), in ascending k, onto an accumulator that starts at +0.0f. A phase without a tap (ntaps < sps) gives +0.0f.
 *   x[j] for j < 0 is the stream's history: the symbols of earlier calls, zeros after create / reset.
 * n_syms symbols in give exactly n_syms sps samples out. The stage delays the signal by (ntaps - 1) / 2 samples and drops nothing: a
 * caller flushes by feeding `history` zero symbols. However a stream is cut into calls, the bits are those of one call.
 * A handle works on a batch of independent streams and keeps each stream's history (the last ceil(ntaps / sps) - 1 symbols) on the
 * device. Stream s of a call reads n_syms symbols at d_in + s in_stride and writes n_syms sps samples at d_out + s out_stride; data are
 * interleaved (re, im) floats as for dvbs2_rotator_*, strides count complex elements and matter only when n_streams > 1. Buffers are
 * 8-byte aligned; an output whose streams all start 16-byte aligned gets 16-byte stores, any other an 8-byte path with the same bits.
 * Input and output must NOT overlap; this is not detected. Two launches per call (the samples, then the new histories), no allocation,
 * no host synchronisation. ONE CALL IN FLIGHT PER HANDLE: a call reads the histories and rewrites them behind itself, so calls on one
 * HIP stream may follow each other, and a call on another HIP stream needs the previous one to have finished. The kernel works in tiles
 * of DVBS2_PULSE_TILE symbols per workgroup.
 * Refused with DVBS2_ESIZE: n_syms > max_symbols, n_streams > max_streams. Refused with DVBS2_EINVAL and a text that names the argument:
 * negative counts, a null buffer with n_syms > 0, with n_streams > 1 an in_stride < n_syms or an out_stride < n_syms sps. n_syms == 0 is
 * a successful call that does nothing. Creation refuses (DVBS2_EINVAL) sps that is not an even integer in 2..64, ntaps < 1 or
 * ceil(ntaps / sps) > 129, a tap that is not finite, max_streams outside 1..65535, max_symbols outside 1..2^30.
 * Host only, no device needed: dvbs2_pulse_geometry (ntaps = 2 sps rrc_delay + 1, history = ceil(ntaps / sps) - 1 = 2 rrc_delay symbols,
 * delay = sps rrc_delay samples; sps an even integer in 2..64, rrc_delay in 1..64, as for dvbs2_symsync_geometry), dvbs2_pulse_taps
 * (h[i] = rrc((i - (ntaps - 1) / 2) / sps - tau, rolloff) gain / S, rrc the closed form behind dvbs2_symsync_taps and S the sum of the
 * taps at tau = 0: the taps sum to gain at tau = 0 -- firdes's convention is gain = sps -- and tau, in symbols, |tau| <= 0.5, only
 * shifts the pulse: a static timing offset; rolloff in [0, 1], gain finite and not zero; designed in double, rounded once) and
 * dvbs2_pulse_scale_taps (the rule of scale_rrc_taps, in place: every tap times sqrt(2) fullscale / max over p < sps of the sum over k of
 * |h[p + k sps]|, in double, rounded once). ---- */
typedef struct dvbs2_pulse dvbs2_pulse_t;
#define DVBS2_PULSE_TILE 512
int dvbs2_pulse_geometry(int sps, int rrc_delay, int* ntaps, int* history, int* delay);
int dvbs2_pulse_taps(int sps, float rolloff, int rrc_delay, double tau, double gain, float* taps);
int dvbs2_pulse_scale_taps(float* taps, int ntaps, int sps, double fullscale);
/* the library's design: dvbs2_pulse_taps with tau = 0 and gain = sps */
int dvbs2_pulse_create(dvbs2_pulse_t** h, int sps, float rolloff, int rrc_delay, int max_streams, int max_symbols, int device);
/* a caller's taps (firdes's own, scaled or shifted ones): any ntaps >= 1 with ceil(ntaps / sps) <= 129, every tap finite */
int dvbs2_pulse_create_taps(dvbs2_pulse_t** h, int sps, const float* taps, int ntaps, int max_streams, int max_symbols, int device);
void dvbs2_pulse_destroy(dvbs2_pulse_t* h);
/* every history back to zeros; synchronous (waits for the device) */
int dvbs2_pulse_reset(dvbs2_pulse_t* h);
/* each nullable; history in symbols, delay = (ntaps - 1) / 2 in samples */
int dvbs2_pulse_params(const dvbs2_pulse_t* h, int* sps, int* ntaps, int* history, int* delay);
/* DEVICE pointers, asynchronous on `stream` */
int dvbs2_pulse_shape_device(dvbs2_pulse_t* h, const float* d_in, int64_t in_stride, int n_syms, int n_streams, float* d_out,
                             int64_t out_stride, void* stream);
/* host pointers, synchronous: stream 0 of the handle, staged through buffers of the handle */
int dvbs2_pulse_shape(dvbs2_pulse_t* h, const float* in, int n_syms, float* out);

/* ---- arbitrary-rate resampling: a polyphase filter bank of `nfilts` branches with linear interpolation between neighbouring branches
 * through a bank of derivative taps, real taps over complex samples. Three uses: the fractional-sps branch of the reference's transmit
 * flowgraph (apps/dvbs2-tx:641-686, GNU Radio's pfb_arb_resampler_ccf(sps, rrc_taps) with 32 branches, behind the PL framer in place of
 * dvbs2_pulse_*), a sampling-clock offset of some ppm in a channel model (the impairment dvbs2_symsync_* tracks), and bringing a capture
 * at, say, 2.5 samples per symbol to the 2 or 4 that dvbs2_symsync_* accepts. pfb_arb_resampler_ccf is not in the reference tree: the
 * stage is UNPINNED against it. What is defined, and tested bit for bit against a float32 restatement (tests/resamp_model.py), is this:
 *   POSITION, in integers and closed form. `step` is a 64-bit count of input samples per output sample with 32 fractional bits, in
 *   [2^26, 2^33]; the rate is exactly 2^32 / step. dvbs2_resamp_step gives nearbyint(2^32 / rate) in double for rate in [0.5, 64]. Each
 *   stream has a 64-bit acc, zero after create / reset. Output m (0-based in a call) of a call of n_in samples sits at T = acc + m step;
 *   with N = n_in << 32 the call writes every m with T < N: n_out = 0 if acc >= N, else ceil((N - acc) / step), and afterwards
 *   acc' = acc + n_out step - N. So the pieces of a stream give the samples of one call, and nothing drifts however long it runs.
 *   From T: i = T >> 32 is the newest input sample used (0-based in the call's input), f = T & 0xffffffff the fraction, branch
 *   j = f >> (32 - log2 nfilts), and a = float((f << log2 nfilts) >> 8) * 2^-24 on 32-bit words, the next 24 bits below the branch bits.
 *   ARITHMETIC. Prototype taps h[0 .. ntaps), derivative taps d[n] = h[n + 1] - h[n] (n < ntaps - 1), d[ntaps - 1] = 0, one float
 *   subtraction each, made at create (the rule of GNU Radio's create_diff_taps). For an output at (i, j, a), real and imaginary part
 *   apart: o0 = sum over k of h[j + k nfilts] x[i - k], o1 = sum over k of d[j + k nfilts] x[i - k], k ascending from 0 while
 *   j + k nfilts < ntaps, each term a float product and then a float addition (no fused multiply-add) onto an accumulator that starts at
 *   +0.0f; then y = o0 + a * o1, a product and then an addition. x before the call is the stream's history: the last
 *   L - 1 = ceil(ntaps / nfilts) - 1 samples of earlier calls, zeros after create / reset.
 * The signal is delayed by ((ntaps - 1) / 2) / nfilts input samples. The taps are the caller's (dvbs2_pulse_taps(nfilts, rolloff, D, 0,
 * nfilts) is the transmit prototype of apps/dvbs2-tx:669-676; with a wide rolloff the same call is a usable interpolation low-pass for a
 * signal at 2 samples per symbol). One rate per handle; dvbs2_resamp_set_rate / _set_step take effect at the next call with acc carried
 * over, so a drifting clock is a sequence of calls.
 * The host keeps a mirror of every acc (plain integer arithmetic): dvbs2_resamp_produce says, without a synchronisation and without
 * advancing anything, what the next call of n_in samples writes per stream; the call reports the same numbers through n_out_host
 * (nullable, n_streams values); dvbs2_resamp_state copies the DEVICE's positions back (synchronous, max_streams values).
 * Stream s of a call reads n_in samples at d_in + s in_stride and writes n_out[s] samples at d_out + s out_stride; data are interleaved
 * (re, im) floats, strides count complex elements, buffers are 8-byte aligned and must NOT overlap (not detected). in_stride matters when
 * n_streams > 1; out_stride is also the capacity of every stream's output and must be at least the call's largest n_out. At most two
 * launches per call (the samples, then the new histories and positions), no allocation, no host synchronisation. ONE CALL IN FLIGHT PER
 * HANDLE, as for dvbs2_pulse_*. The kernel works in tiles of DVBS2_RESAMP_TILE output samples per workgroup.
 * Refused with DVBS2_ESIZE: n_in > max_samples, n_streams > max_streams. Refused with DVBS2_EINVAL and a text that names the argument:
 * negative counts, a null buffer with n_in > 0, buffers that are not 8-byte aligned, with n_streams > 1 an in_stride < n_in, an
 * out_stride (host entry: out_cap) below the largest n_out. A refused call leaves output, histories, positions and mirror untouched.
 * n_in == 0 is a successful call that does nothing. Creation refuses (DVBS2_EINVAL) nfilts that is not a power of two in 2..256, ntaps
 * outside 1..8192 or ceil(ntaps / nfilts) > 128, a tap that is not finite, a rate outside [0.5, 64], max_streams outside 1..65535,
 * max_samples outside 1..2^24 (with that cap nothing overflows 64 bits and n_out < 2^31).
 * Host only, no device needed: dvbs2_resamp_step, dvbs2_resamp_geometry (terms = L, history = L - 1, delay_num = (ntaps - 1) / 2),
 * dvbs2_resamp_max_out (ceil((n_in << 32) / step): the largest n_out of a call of n_in samples for any acc; negative on a bad argument)
 * and dvbs2_resamp_check (the argument check of dvbs2_resamp_create). ---- */
typedef struct dvbs2_resamp dvbs2_resamp_t;
#define DVBS2_RESAMP_TILE 1024
int dvbs2_resamp_step(double rate, uint64_t* step);
int dvbs2_resamp_geometry(int nfilts, int ntaps, int* terms, int* history, int* delay_num);
int64_t dvbs2_resamp_max_out(uint64_t step, int n_in);
int dvbs2_resamp_check(int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples);
int dvbs2_resamp_create(dvbs2_resamp_t** h, int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples,
                        int device);
void dvbs2_resamp_destroy(dvbs2_resamp_t* h);
/* every history and position back to zero; synchronous (waits for the device) */
int dvbs2_resamp_reset(dvbs2_resamp_t* h);
/* acc[s] = frac[s] for each of the handle's max_streams streams (null: zeros); histories stay; synchronous */
int dvbs2_resamp_reset_phase(dvbs2_resamp_t* h, const uint32_t* frac);
int dvbs2_resamp_set_rate(dvbs2_resamp_t* h, double rate);
int dvbs2_resamp_set_step(dvbs2_resamp_t* h, uint64_t step);
/* each nullable */
int dvbs2_resamp_params(const dvbs2_resamp_t* h, int* nfilts, int* ntaps, int* terms, int* history, int* delay_num, uint64_t* step);
int dvbs2_resamp_produce(const dvbs2_resamp_t* h, int n_in, int n_streams, int64_t* n_out);
int dvbs2_resamp_state(dvbs2_resamp_t* h, uint64_t* acc);
/* DEVICE pointers, asynchronous on `stream`; n_out_host is a HOST array, filled before the call returns */
int dvbs2_resamp_process_device(dvbs2_resamp_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out,
                                int64_t out_stride, int64_t* n_out_host, void* stream);
/* host pointers, synchronous: stream 0 of the handle, staged through buffers of the handle; out_cap in complex elements */
int dvbs2_resamp_process(dvbs2_resamp_t* h, const float* in, int n_in, float* out, int64_t out_cap, int64_t* n_out);

/* ---- digital down-conversion: a frequency-translating decimating FIR with real taps, the way from a wideband capture to baseband
 * streams at 2 samples per symbol. One handle turns up to max_inputs sample streams into up to max_channels channels: channel c reads
 * input stream input[c] (0 until set), mixes it with its own phase increment inc[c] (radians per input sample, 0 until set), filters it
 * with the handle's taps h[0 .. ntaps) and keeps every decim-th sample. It is GNU Radio's freq_xlating_fir_filter_ccf, or a rotator
 * followed by fir_filter_ccf with decimation; neither is in the reference tree: the stage is UNPINNED against it. It is the mirror image
 * of dvbs2_pulse_* and reuses the phase of dvbs2_rotator_*. What is defined, and tested bit for bit against a float32 restatement
 * (tests/ddc_model.py) applied to the output of dvbs2_rotator_rotate_device, is this:
 *   MIX. z[n] = x[n] e^{j phi_c(n)} with the rotator's arithmetic: the phase in turns as unsigned 64-bit fixed point,
 *   phi_c(n) = P_c + (n - n_call) I_c in wrapping integer arithmetic, n_call the first sample of the call, I_c the increment converted
 *   once as the rotator converts it; the upper 32 bits as a float in half-turns go to sincospif; four products, a subtraction, an
 *   addition, nothing fused. inc == 0 is no special case.
 *   FILTER AND DECIMATE. Output k (absolute, k >= 0) is y[k] = sum over t = 0 .. ntaps - 1 of h[t] z[k decim - t], real and imaginary
 *   part apart, each term a float product and then a float addition, t ascending, onto an accumulator that starts at +0.0f. z[n] for
 *   n < 0 is zero after create / reset.
 *   COUNTS. All inputs and channels of a handle share one 64-bit sample counter n0, zero after create / reset; every input stream of a
 *   call has n_in samples. The call writes, for every channel, the outputs k with n0 <= k decim < n0 + n_in:
 *   n_out = ceil((n0 + n_in) / decim) - ceil(n0 / decim), and leaves n0' = n0 + n_in and P_c' = P_c + n_in I_c for the channels of the
 *   call. The first output of a stream uses its first sample.
 *   STATE. Per channel the last ntaps - 1 MIXED samples stay on the device, so the stage equals "rotator, then decimating FIR" bit for
 *   bit however the stream is cut into calls and whenever increments change between calls (dvbs2_ddc_set_channel: from the next call
 *   on, the phase continuous). A call on fewer than max_channels channels leaves the state of the others alone.
 * The signal is delayed by (ntaps - 1) / 2 input samples (delay_num = ntaps - 1 halves of an input sample). The taps are the caller's:
 * with decim = sps / 2, dvbs2_pulse_taps(sps, rolloff, D, 0, 1) is the matched filter of a carrier at sps samples per symbol.
 * The host keeps a mirror of the counter and of every phase (plain integer arithmetic): dvbs2_ddc_position and dvbs2_ddc_channel read
 * it, and the call reports n_out (nullable), all without a synchronisation; dvbs2_ddc_state copies the DEVICE's phases back
 * (synchronous, max_channels values).
 * Channel c of a call reads n_in samples at d_in + input[c] in_stride and writes n_out samples at d_out + c out_stride; data are
 * interleaved (re, im) floats, strides count complex elements, buffers are 8-byte aligned and must NOT overlap (not detected); the input
 * is never written. in_stride matters when n_inputs > 1; out_stride is also the capacity of every channel's output. Two launches per
 * call (the samples, then the new histories and phases; the first call behind a dvbs2_ddc_set_channel also copies the channel table on
 * the stream), no allocation, no host synchronisation. ONE CALL IN FLIGHT PER HANDLE, as for dvbs2_pulse_*. A workgroup writes
 * min(DVBS2_DDC_MAX_TILE, (DVBS2_DDC_SPAN - (ntaps - 1)) / decim) consecutive output samples of one channel.
 * Refused with DVBS2_ESIZE: n_in > max_samples, n_inputs > max_inputs, n_channels > max_channels. Refused with DVBS2_EINVAL and a text
 * that names the argument: negative counts, a null buffer with n_in > 0 and n_channels > 0, buffers that are not 8-byte aligned, with
 * n_inputs > 1 an in_stride < n_in, an out_stride < n_out, a channel of the call whose input is not below n_inputs. A refused call leaves
 * output, histories, phases and mirror untouched. n_in == 0 is a successful call that does nothing; n_channels == 0 only advances the
 * counter. Creation refuses (DVBS2_EINVAL) decim outside 1..256, ntaps outside 1..4096, a tap that is not finite, max_channels or
 * max_inputs outside 1..65535, max_samples outside 1..2^24.
 * Host only, no device needed: dvbs2_ddc_geometry (history = ntaps - 1, delay_num = ntaps - 1; each nullable), dvbs2_ddc_produce (the
 * count rule for a counter at `position`; -1 when position is negative or above 2^62, decim or n_in out of range) and dvbs2_ddc_check
 * (the argument check of dvbs2_ddc_create). ---- */
typedef struct dvbs2_ddc dvbs2_ddc_t;
#define DVBS2_DDC_SPAN 9216
#define DVBS2_DDC_MAX_TILE 1024
int dvbs2_ddc_geometry(int decim, int ntaps, int* history, int* delay_num);
int64_t dvbs2_ddc_produce(int64_t position, int decim, int n_in);
int dvbs2_ddc_check(int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples);
int dvbs2_ddc_create(dvbs2_ddc_t** h, int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples,
                     int device);
void dvbs2_ddc_destroy(dvbs2_ddc_t* h);
/* counter 0, phases 0, histories zero; the channel table (inputs and increments) stays; synchronous (waits for the device) */
int dvbs2_ddc_reset(dvbs2_ddc_t* h);
/* host only; phase_inc in radians per input sample, any finite value */
int dvbs2_ddc_set_channel(dvbs2_ddc_t* h, int channel, int input, double phase_inc);
/* each nullable; tile: output samples per workgroup */
int dvbs2_ddc_params(const dvbs2_ddc_t* h, int* decim, int* ntaps, int* history, int* delay_num, int* tile);
/* host only, from the mirror */
int dvbs2_ddc_position(const dvbs2_ddc_t* h, int64_t* counter);
/* host only, from the mirror, each nullable: the channel's input, its increment and its phase in 2^-64 turns */
int dvbs2_ddc_channel(const dvbs2_ddc_t* h, int channel, int* input, uint64_t* inc_turns, uint64_t* phase_turns);
int dvbs2_ddc_state(dvbs2_ddc_t* h, uint64_t* phases);
/* DEVICE pointers, asynchronous on `stream`; n_out is a HOST value, filled before the call returns */
int dvbs2_ddc_process_device(dvbs2_ddc_t* h, const float* d_in, int64_t in_stride, int n_in, int n_inputs, int n_channels, float* d_out,
                             int64_t out_stride, int64_t* n_out, void* stream);
/* host pointers, synchronous, staged through buffers of the handle; the same arguments and checks */
int dvbs2_ddc_process(dvbs2_ddc_t* h, const float* in, int64_t in_stride, int n_in, int n_inputs, int n_channels, float* out,
                      int64_t out_stride, int64_t* n_out);

/* ---- spectrum estimate and carrier finder: what tells dvbs2_ddc_set_channel, the down-converter's decimation and dvbs2_pulse_taps
 * where the carriers of a capture sit. Power spectra by Welch's method (windowed, overlapped segments, averaged periodograms), the data
 * of GNU Radio's freq_sink_c and waterfall_sink_c; neither is in the reference tree: the stage is UNPINNED against it. A handle holds
 * nfft = 2^t (t in 6..13), hop (1..2^24), avg (>= 0), a real window of nfft floats (null: periodic Hann) and the bin order; it holds NO
 * signal state: a call is a pure function of its input. What is defined, and tested bit for bit against a float32 restatement
 * (tests/spectrum_model.py), is this:
 *   SEGMENTS. Segment s of a stream is the call's samples [s hop, s hop + nfft); n_seg = (n_in - nfft) / hop + 1 for n_in >= nfft,
 *   else 0. With avg > 0 a row is avg consecutive segments, n_rows = n_seg / avg, and what is left over is not used; with avg == 0 the
 *   call's segments form one row. dvbs2_spectrum_geometry gives the counts before the call.
 *   WINDOW. xw = (re w[n], im w[n]), one float product each.
 *   TRANSFORM. X[k] = sum_n xw[n] e^{-2 pi j k n / nfft} as the radix-2 decimation-in-time graph over the bit-reversed input: stage
 *   s = 1..t pairs i and i + 2^(s-1), (a, b) -> (a + T, a - T), T = W b, W entry (i mod 2^(s-1)) nfft / 2^s of ONE table of nfft / 2
 *   entries (float(cos(2 pi i / nfft)), float(-sin(2 pi i / nfft))), computed in double (dvbs2_spectrum_twiddles). Stage 1 has no
 *   product; every later stage does Tr = Wr br - Wi bi, Ti = Wr bi + Wi br for every index, nothing fused.
 *   POWER AND AVERAGE. p = Xr Xr + Xi Xi. The segments of a row are cut into chunks of DVBS2_SPECTRUM_CHUNK consecutive segments; a
 *   chunk's sum per bin is float additions in ascending segment order onto +0.0f, the row is the chunk sums added in ascending order
 *   onto +0.0f, then one float product with scale = float(1 / (n sum w[n]^2)), n the row's segment count, in double on the host. White
 *   noise of variance sigma^2 gives sigma^2 in every bin.
 *   OUTPUT. Row r of stream i is nfft floats at d_out + i out_stride + r nfft: bins 0..nfft-1, DC first, or with shifted != 0 bins
 *   nfft/2..nfft-1, 0..nfft/2-1, DC at index nfft/2. Non-finite input propagates as IEEE says; denormals are kept.
 * Stream i reads n_in interleaved (re, im) samples at d_in + i in_stride (complex elements, 8-byte aligned); out_stride counts floats
 * (4-byte aligned) and is also the capacity of a stream's rows. Two launches at most, no allocation, no host synchronisation; the chunk
 * sums of a call live in a buffer of the handle sized at create from max_streams and max_samples: ONE CALL IN FLIGHT PER HANDLE.
 * Refused with DVBS2_ESIZE: n_in > max_samples, n_streams > max_streams. Refused with DVBS2_EINVAL and a text that names the argument:
 * negative counts, a null or misaligned buffer where something is to be written, with n_streams > 1 an in_stride < n_in, an out_stride
 * < n_rows nfft. A refused call writes nothing. n_in < nfft (or fewer than avg segments) is a successful call with n_rows == 0 that
 * writes nothing. Creation refuses (DVBS2_EINVAL) an nfft that is no power of two in 64..8192, hop outside 1..2^24, a negative avg, a
 * window value that is not finite, a window of zeros, max_streams outside 1..65535, max_samples outside 1..2^24.
 * Host only, no device needed: dvbs2_spectrum_geometry (each output nullable; used_samples is one past the last sample a row reads),
 * dvbs2_spectrum_window (periodic rectangular, Hann, Hamming and 4-term Blackman-Harris windows, evaluated in double and rounded
 * once), dvbs2_spectrum_twiddles (nfft / 2 (re, im) pairs), dvbs2_spectrum_check (the argument check of dvbs2_spectrum_create) and
 * dvbs2_spectrum_carriers.
 * CARRIER FINDER. One row in double arithmetic, deterministic (tests/spectrum_model.py restates it). The row is smoothed by a circular
 * moving average of `smooth` bins (odd); the noise floor is the element floor(floor_quantile (nfft - 1)) of the sorted smoothed row;
 * regions are circular runs of bins above floor 10^(threshold_db / 10), so a carrier across the band edge is one region; regions with
 * fewer than min_gap bins between them become one and regions of fewer than min_width bins are dropped. Per region: `centre` in cycles
 * per sample in [-0.5, 0.5), the centroid of (smoothed - floor) over the region and its skirts (outwards on either side while the
 * difference stays positive, at most half way to the neighbouring region); `level`, the median of (smoothed - floor) over the region's middle
 * half; `bandwidth` in cycles per sample between the two half-level crossings, linearly interpolated; `floor`; the two edge bins as
 * indices of the caller's row. A root-raised-cosine carrier's power spectrum is at half its plateau at +-Rs / 2 for any roll-off:
 * bandwidth is the symbol rate, 1 / bandwidth the samples per symbol, -2 pi centre the phase_inc of dvbs2_ddc_set_channel.
 * params == NULL: smooth 9, floor_quantile 0.25, threshold_db 6, min_gap 4, min_width 8. Records come sorted by centre; *n_found is
 * the number found, of which the first max_out are written. Refused: values that are negative or not finite in the row, nfft no power
 * of two in 16..2^20, smooth even or outside 1..nfft/2, floor_quantile outside 0..1, threshold_db outside (0, 200], min_gap or
 * min_width outside 1..nfft. ---- */
typedef struct dvbs2_spectrum dvbs2_spectrum_t;
#define DVBS2_SPECTRUM_CHUNK 16
#define DVBS2_SPECTRUM_RECT 0
#define DVBS2_SPECTRUM_HANN 1
#define DVBS2_SPECTRUM_HAMMING 2
#define DVBS2_SPECTRUM_BLACKMAN_HARRIS 3
typedef struct { double floor_quantile, threshold_db; int32_t smooth, min_gap, min_width, reserved; } dvbs2_spectrum_carrier_params_t;
typedef struct { double centre, bandwidth, level, floor; int32_t lo_bin, hi_bin; } dvbs2_spectrum_carrier_t;
int dvbs2_spectrum_geometry(int nfft, int hop, int avg, int n_in, int* n_seg, int* n_rows, int* used_samples);
int dvbs2_spectrum_window(int kind, int nfft, float* out);
int dvbs2_spectrum_twiddles(int nfft, float* out);
int dvbs2_spectrum_check(int nfft, int hop, int avg, const float* window, int max_streams, int max_samples);
int dvbs2_spectrum_carriers(const float* psd, int nfft, int shifted, const dvbs2_spectrum_carrier_params_t* params,
                            dvbs2_spectrum_carrier_t* out, int max_out, int* n_found);
int dvbs2_spectrum_create(dvbs2_spectrum_t** h, int nfft, int hop, int avg, const float* window, int shifted, int max_streams,
                          int max_samples, int device);
void dvbs2_spectrum_destroy(dvbs2_spectrum_t* h);
/* each nullable; window_power: sum w[n]^2 in double, ascending n */
int dvbs2_spectrum_params(const dvbs2_spectrum_t* h, int* nfft, int* hop, int* avg, int* shifted, double* window_power);
/* DEVICE pointers, asynchronous on `stream`; n_rows is a HOST value (nullable), known before anything is launched */
int dvbs2_spectrum_process_device(dvbs2_spectrum_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out,
                                  int64_t out_stride, int* n_rows, void* stream);
/* host pointers, synchronous, staged through buffers of the handle; the same arguments and checks, alignment apart */
int dvbs2_spectrum_process(dvbs2_spectrum_t* h, const float* in, int64_t in_stride, int n_in, int n_streams, float* out,
                           int64_t out_stride, int* n_rows);

/* ---- polyphase filter bank channelizer: a capture split into M equally spaced carriers, the FIR work done ONCE for all channels and one
 * M-point transform in place of M mixers. It is GNU Radio's pfb_channelizer_ccf; the block is not in the reference tree: the stage is
 * UNPINNED against it. A handle holds n_chan = M (a power of two in 2..256), decim = D (1..M, any integer, not only a divisor of M),
 * ntaps (1..4096) real taps h, a selection of channels (all M ascending until set), ONE 64-bit absolute sample counter n0 for all
 * streams, and per stream the last ntaps - 1 RAW input samples; x[n] for n < 0 is zero after create / reset. What is defined, and tested
 * bit for bit against a float32 restatement (tests/pfbch_model.py), is this:
 *   COUNTS. The down-converter's: a call over the absolute inputs [n0, n0 + n_in) writes the outputs k with n0 <= k D < n0 + n_in,
 *   n_out = ceil((n0 + n_in) / D) - ceil(n0 / D) per channel, and leaves n0' = n0 + n_in. n_in in 0..2^24, n0 at most 2^62.
 *   BRANCH SUMS. For output k and residue r in 0..M-1: w[k][r] = sum over the taps t with (k D - t) mod M == r of h[t] x[k D - t], t
 *   ascending, real and imaginary part apart, each term a float product and then a float addition onto +0.0f, nothing fused. A residue
 *   without a tap (ntaps < M) is +0.0f. The residue is that of the ABSOLUTE sample index, so nothing depends on how a stream is cut.
 *   TRANSFORM. Y[k][c] = sum_r w[k][r] e^{-2 pi j c r / M} by the graph of dvbs2_spectrum_*: input to bit-reversed places, stages
 *   s = 1..log2 M, (a, b) -> (a + T, a - T), stage 1 with T = b, every later stage Tr = Wr br - Wi bi, Ti = Wr bi + Wi br for EVERY
 *   index (unit twiddles included), W from one table of M / 2 entries (float(cos(2 pi i / M)), float(-sin(2 pi i / M))) computed in
 *   double: dvbs2_pfbch_twiddles, the entries of dvbs2_spectrum_twiddles for 2..256.
 *   MEANING. Y[k][c] = sum_t h[t] x[k D - t] e^{-2 pi j c (k D - t) / M}: channel c is the band centred at +c / M of the input rate (the
 *   upper half of the indices are the negative frequencies), filtered by h and output at 1 / D of the input rate. In exact arithmetic
 *   it is dvbs2_ddc_* from reset with phase_inc = -2 pi c / M, the same taps and the same decim. The delay is (ntaps - 1) / 2 input
 *   samples (delay_num = ntaps - 1 halves of one).
 *   OUTPUT. Row i of stream s is n_out complex samples at d_out + (s n_sel + i) out_stride and holds channel list[i].
 *   dvbs2_pfbch_set_channels (host only) accepts 1..M distinct indices in any order and takes effect from the next call; channels that
 *   are not selected are not written. The transform is computed whole.
 *   STATE. Raw history only, no phases: cuts of any kind -- empty calls, calls shorter than D or than the history, a changed selection
 *   between calls -- give the bits of one call.
 * Stream s reads n_in interleaved (re, im) samples at d_in + s in_stride; strides count complex elements, buffers are 8-byte aligned;
 * in == out is refused and other overlaps are not detected. in_stride matters when n_streams > 1; out_stride is also the capacity of
 * every row. Two launches per call at most (the samples, then the new histories; the first call behind a dvbs2_pfbch_set_channels also
 * copies the selection on the stream), no allocation, no host synchronisation; the counter is mirrored on the host, so
 * dvbs2_pfbch_position and the reported n_out (nullable) need none. ONE CALL IN FLIGHT PER HANDLE. A workgroup writes
 * min(DVBS2_PFBCH_MAX_TILE, (DVBS2_PFBCH_SPAN - (ntaps - 1) - n_chan) / decim) consecutive output instants of one stream.
 * Refused with DVBS2_ESIZE: n_in > max_samples, n_streams > max_streams. Refused with DVBS2_EINVAL and a text that names the argument:
 * negative counts, a null buffer with n_in > 0 and n_streams > 0, in == out, with n_streams > 1 an in_stride < n_in, an out_stride
 * < n_out (checked before anything is launched), buffers that are not 8-byte aligned, a selection that is null, empty, longer than
 * n_chan, out of range or repeating. A refused call leaves output, histories, counter and selection untouched. n_in == 0 is a
 * successful call that does nothing; n_streams == 0 only advances the counter. That does not cover a DVBS2_EDEVICE between the two launches
 * (the first accepted, the second not): the outputs are then written, histories and counter are not advanced, and the handle is to be
 * reset. Creation refuses (DVBS2_EINVAL) an n_chan that is no
 * power of two in 2..256, decim outside 1..n_chan, ntaps outside 1..4096, a tap that is not finite, max_streams outside 1..65535,
 * max_samples outside 1..2^24.
 * Host only, no device needed: dvbs2_pfbch_geometry (history = ntaps - 1, delay_num = ntaps - 1, taps_per_branch = ceil(ntaps /
 * n_chan); each nullable), dvbs2_pfbch_produce (the count rule; decim in 1..256), dvbs2_pfbch_twiddles (n_chan / 2 (re, im) pairs),
 * dvbs2_pfbch_check (the argument check of dvbs2_pfbch_create), dvbs2_pfbch_set_channels, dvbs2_pfbch_channels (list: room for n_chan
 * values; each nullable), dvbs2_pfbch_params, dvbs2_pfbch_position. ---- */
typedef struct dvbs2_pfbch dvbs2_pfbch_t;
#define DVBS2_PFBCH_SPAN 5376
#define DVBS2_PFBCH_MAX_TILE 1024
int dvbs2_pfbch_geometry(int n_chan, int decim, int ntaps, int* history, int* delay_num, int* taps_per_branch);
int64_t dvbs2_pfbch_produce(int64_t position, int decim, int n_in);
int dvbs2_pfbch_twiddles(int n_chan, float* out);
int dvbs2_pfbch_check(int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples);
int dvbs2_pfbch_create(dvbs2_pfbch_t** h, int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples, int device);
void dvbs2_pfbch_destroy(dvbs2_pfbch_t* h);
/* counter 0, histories zero; the selection stays; synchronous (waits for the device) */
int dvbs2_pfbch_reset(dvbs2_pfbch_t* h);
int dvbs2_pfbch_set_channels(dvbs2_pfbch_t* h, const int* list, int n_sel);
/* each nullable; tile: output instants per workgroup */
int dvbs2_pfbch_params(const dvbs2_pfbch_t* h, int* n_chan, int* decim, int* ntaps, int* history, int* delay_num, int* tile);
int dvbs2_pfbch_position(const dvbs2_pfbch_t* h, int64_t* counter);
int dvbs2_pfbch_channels(const dvbs2_pfbch_t* h, int* list, int* n_sel);
/* DEVICE pointers, asynchronous on `stream`; n_out is a HOST value, filled before the call returns */
int dvbs2_pfbch_process_device(dvbs2_pfbch_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out,
                               int64_t out_stride, int64_t* n_out, void* stream);
/* host pointers, synchronous, staged through buffers of the handle; the same arguments and checks, alignment apart */
int dvbs2_pfbch_process(dvbs2_pfbch_t* h, const float* in, int64_t in_stride, int n_in, int n_streams, float* out, int64_t out_stride,
                        int64_t* n_out);

/* ---- polyphase SYNTHESIS filter bank, the transpose of dvbs2_pfbch_*: the rows of M equally spaced channels become one wideband stream
 * at L times their rate, with ONE M-point inverse transform per input instant in place of M mixers and ONE FIR pass for all channels.
 * It is GNU Radio's pfb_synthesizer_ccf; the block is not in the reference tree: the stage is UNPINNED against it. With interp = M and
 * root-raised-cosine taps it takes the PLFRAME symbols of M carriers straight to the wideband stream (pulse shaper, mixers and sum in
 * one stage). A handle holds n_chan = M (a power of two in 2..256), interp = L (1..M, any integer, not only a divisor of M), ntaps
 * (1..4096) real finite taps h, a selection of channels (all M ascending until set), ONE 64-bit counter k0 of input INSTANTS for all
 * streams (at most 2^54), and per stream a TAIL of max(ntaps - L, 0) complex partial sums, zero after create / reset. What is defined,
 * and tested bit for bit against a float32 restatement (tests/pfbsyn_model.py), is this:
 *   COUNTS. A call of n_in instants (0..max_samples) reads n_in samples from each of the n_sel rows of a stream and writes exactly
 *   n_out = n_in L samples per stream, the absolute outputs n in [k0 L, (k0 + n_in) L); then k0' = k0 + n_in.
 *   INPUT. Row i of stream s is at d_in + (s n_sel + i) in_stride and feeds channel list[i]; dvbs2_pfbsyn_set_channels (host only)
 *   accepts 1..M distinct indices in any order and takes effect from the next call. A channel without a row is +0.0f in both parts.
 *   Stream s writes at d_out + s out_stride.
 *   TRANSFORM. For instant k with inputs a[c]: v[k][r] = sum_c a[c] e^{+2 pi j c r / M}, r = 0..M-1, unnormalised, on the graph and
 *   the one table of dvbs2_spectrum_* / dvbs2_pfbch_* (dvbs2_pfbch_twiddles): the graph's input is (re, im) := (a.im, a.re) with
 *   channel c at its bit-reversed place, stage 1 has no product, every later stage computes Tr = Wr br - Wi bi, Ti = Wr bi + Wi br for
 *   EVERY index, nothing is fused, and the result is read as (v.im, v.re) := (re, im).
 *   FIR. For the absolute output n let r = n mod M, p = n mod L, k1 = n div L. Over the j with t = p + j L <= ntaps - 1 and
 *   k = k1 - j >= 0, j DESCENDING (the oldest instant first; the channelizer's order is the opposite): acc = acc + h[t] * v[k][r] from
 *   +0.0f, real and imaginary part apart, the product rounded to float and then the addition. An instant that does not exist (k < 0
 *   after a reset) is skipped, not multiplied by zero.
 *   TAIL. After a call tail[i] holds, for output k0' L + i, the acc over the instants k < k0' (+0.0f where there is none). The next
 *   call starts those outputs from the tail and goes on with its own instants: cuts of any kind -- empty calls, calls of one instant,
 *   calls shorter than the tail, a changed selection between calls -- give the bits of one call. Every instant is synthesised with
 *   the selection of its own call.
 *   MEANING. y[n] = sum_c e^{+2 pi j c n / M} sum_k h[n - k L] x_c[k]: every row shaped by an interpolating FIR by L (the
 *   dvbs2_pulse_* sum, for any L), moved by dvbs2_rotator_* with +2 pi c / M from phase 0 at n = 0, and the rows added. Channel c is
 *   the band centred at +c / M of the OUTPUT rate, the channelizer's numbering: dvbs2_pfbch_* with (M, L, g) on the output returns row
 *   c as x_c through h * g at the instants k L. The delay is (ntaps - 1) / 2 output samples (delay_num = ntaps - 1 halves of one).
 * Strides count complex elements, buffers are 8-byte aligned; in == out is refused and other overlaps are not detected. in_stride
 * matters when the call has more than one row. Two launches per call at most (the samples and the tails the call leaves, then those
 * tails copied over the old ones; the first call behind a dvbs2_pfbsyn_set_channels also copies the selection on the stream), no
 * allocation, no host synchronisation; the counter is mirrored on the host, so dvbs2_pfbsyn_position and the reported n_out
 * (nullable) need none. ONE CALL IN FLIGHT PER HANDLE. A workgroup owns dvbs2_pfbsyn_tile(n_chan, interp, ntaps) consecutive
 * instants of one stream: with q = ceil(ntaps / interp) and seg = (n_chan + n_chan / 16) | 1, fit = DVBS2_PFBSYN_SPAN / seg - (q - 1)
 * where that is at least q and DVBS2_PFBSYN_SPAN_LONG / seg - (q - 1) otherwise, DVBS2_PFBSYN_MAX_TILE at most.
 * Refused with DVBS2_ESIZE: n_in > max_samples, n_streams > max_streams. Refused with DVBS2_EINVAL and a text that names the argument:
 * negative counts, a null buffer with n_in > 0 and n_streams > 0, in == out, with more than one row an in_stride < n_in, an out_stride
 * < n_out (checked before anything is launched), buffers that are not 8-byte aligned, a counter that would pass 2^54, a selection that
 * is null, empty, longer than n_chan, out of range or repeating. A refused call leaves output, tails, counter and selection
 * untouched. n_in == 0 is a successful call that does nothing; n_streams == 0 only advances the counter. That does not cover a
 * DVBS2_EDEVICE between the two launches (the first accepted, the second not): the outputs are then written, tails and counter are
 * not advanced, and the handle is to be reset. Creation refuses (DVBS2_EINVAL) an n_chan that is no power of two in 2..256, interp
 * outside 1..n_chan, ntaps outside 1..4096, a tap that is not finite, n_chan * ceil(ntaps / interp) > DVBS2_PFBSYN_MAX_PRODUCT (a
 * workgroup holds the transformed instants that its first output needs on chip: interp = 1 with a long filter on many channels is
 * not a use of this stage), max_streams outside 1..65535, max_samples outside 1..2^24, max_samples * interp > 2^28.
 * Host only, no device needed: dvbs2_pfbsyn_geometry (tail = max(ntaps - interp, 0), delay_num = ntaps - 1, taps_per_phase =
 * ceil(ntaps / interp); each nullable), dvbs2_pfbsyn_tile (the tile, or DVBS2_EINVAL for a shape that creation refuses),
 * dvbs2_pfbsyn_check (the argument check of dvbs2_pfbsyn_create), dvbs2_pfbsyn_set_channels, dvbs2_pfbsyn_channels (list: room for
 * n_chan values; each nullable), dvbs2_pfbsyn_params, dvbs2_pfbsyn_position. ---- */
typedef struct dvbs2_pfbsyn dvbs2_pfbsyn_t;
#define DVBS2_PFBSYN_SPAN 6144
#define DVBS2_PFBSYN_SPAN_LONG 13312
#define DVBS2_PFBSYN_MAX_TILE 512
#define DVBS2_PFBSYN_MAX_PRODUCT 8192
int dvbs2_pfbsyn_geometry(int n_chan, int interp, int ntaps, int* tail, int* delay_num, int* taps_per_phase);
int dvbs2_pfbsyn_tile(int n_chan, int interp, int ntaps);
int dvbs2_pfbsyn_check(int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples);
int dvbs2_pfbsyn_create(dvbs2_pfbsyn_t** h, int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples, int device);
void dvbs2_pfbsyn_destroy(dvbs2_pfbsyn_t* h);
/* counter 0, tails zero; the selection stays; synchronous (waits for the device) */
int dvbs2_pfbsyn_reset(dvbs2_pfbsyn_t* h);
int dvbs2_pfbsyn_set_channels(dvbs2_pfbsyn_t* h, const int* list, int n_sel);
/* each nullable; tile: input instants per workgroup */
int dvbs2_pfbsyn_params(const dvbs2_pfbsyn_t* h, int* n_chan, int* interp, int* ntaps, int* tail, int* delay_num, int* tile);
int dvbs2_pfbsyn_position(const dvbs2_pfbsyn_t* h, int64_t* counter);
int dvbs2_pfbsyn_channels(const dvbs2_pfbsyn_t* h, int* list, int* n_sel);
/* DEVICE pointers, asynchronous on `stream`; n_out is a HOST value, filled before the call returns */
int dvbs2_pfbsyn_process_device(dvbs2_pfbsyn_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out,
                                int64_t out_stride, int64_t* n_out, void* stream);
/* host pointers, synchronous, staged through buffers of the handle; the same arguments and checks, alignment apart */
int dvbs2_pfbsyn_process(dvbs2_pfbsyn_t* h, const float* in, int64_t in_stride, int n_in, int n_streams, float* out, int64_t out_stride,
                         int64_t* n_out);

/* ---- downstream neighbour: BBFRAME de-header, replaces bbdeheader_bb_impl::general_work (reference
 * lib/bbdeheader_bb_impl.cc:144-264) with parse_bbheader (:77-136) and check_crc8 (:138-142, generator
 * x^8 + x^7 + x^6 + x^4 + x^2 + 1, :55). Input: whole descrambled BBFRAMEs of kbch / 8 bytes (what dvbs2_bch_decode /
 * dvbs2_chain_* emit with descrambling on); output: 188-byte MPEG-TS packets back to back, sync byte restored, transport
 * error indicator set where the packet's CRC-8 fails. The block's state -- synchronised flag, the partial TS packet that
 * continues in the next BBFRAME, the five counters -- lives in the handle and carries over from call to call exactly as it
 * carries over between work() calls of the block; dvbs2_bbdeheader_reset() gives the block as constructed.
 * One defined deviation: a header that passes every check but has SYNCD/8 + 1 > DFL/8 while the block re-synchronises makes
 * the reference's unsigned byte count wrap and its loop read past the buffer (:201-202); such a BBFRAME is dropped here and
 * counted in `overruns`.
 * kbch_bits = fec_info.bch_k of (standard, framesize, rate); out capacity >= n_frames * max_out_bytes_per_frame. */
typedef struct dvbs2_bbdeheader dvbs2_bbdeheader_t;
typedef struct {
    uint64_t packets, errors, bbframes, dropped, gaps; /* d_packet_cnt, d_error_cnt, d_bbframe_cnt, d_bbframe_drop_cnt, d_bbframe_gap_cnt */
    uint64_t overruns;
    int32_t synched, partial_ts_bytes;                  /* d_synched, d_partial_ts_bytes */
} dvbs2_bbdeheader_counters_t;
int dvbs2_bbdeheader_create(dvbs2_bbdeheader_t** h, int standard, int framesize, int rate, int max_frames, int device);
int dvbs2_bbdeheader_create_raw(dvbs2_bbdeheader_t** h, int kbch_bits, int max_frames, int device);
void dvbs2_bbdeheader_destroy(dvbs2_bbdeheader_t* h);
int dvbs2_bbdeheader_params(const dvbs2_bbdeheader_t* h, int* kbch_bytes, int* max_dfl_bits, int* max_out_bytes_per_frame);
/* host buffers; *produced = bytes written to ts_out (a multiple of 188) */
int dvbs2_bbdeheader_process(dvbs2_bbdeheader_t* h, const uint8_t* bbframes, int n_frames, uint8_t* ts_out, int64_t* produced);
/* device buffers, asynchronous on `stream`; the byte count of the call is read with dvbs2_bbdeheader_finish */
int dvbs2_bbdeheader_process_device(dvbs2_bbdeheader_t* h, const uint8_t* d_bbframes, int n_frames, uint8_t* d_ts_out, void* stream);
/* waits for the calls enqueued on `stream`; *produced = bytes written by the LAST of them */
int dvbs2_bbdeheader_finish(dvbs2_bbdeheader_t* h, int64_t* produced, void* stream);
int dvbs2_bbdeheader_counters(dvbs2_bbdeheader_t* h, dvbs2_bbdeheader_counters_t* out, void* stream);
int dvbs2_bbdeheader_reset(dvbs2_bbdeheader_t* h, void* stream);

/* ---- de-header rows: the de-header above for a BATCH of streams in a fixed number of launches, from state held in the CALLER'S
 * device memory. There is no handle, and the host reads nothing: not the frame ranges, not the byte counts.
 * FRAMES. Stream s of a call owns the BBFRAMEs d_offsets[s] .. d_offsets[s + 1] of d_bbframes: kbch_bits / 8 bytes each, back to back,
 * stream-major, as dvbs2_chain_* and dvbs2_bch_* write the slots that dvbs2_plsync_batch_gather_device counted. d_offsets (n_streams + 1
 * entries, non-decreasing, d_offsets[n_streams] = the frames of the call) is read on the DEVICE. Frames at or above max_frames are
 * ignored (the rule of dvbs2_rotator_control_device for max_slots): presented again in the next call they give the bytes of one call.
 * Whatever d_offsets holds, device code stays inside its buffers: every offset is clamped to [0, min(d_offsets[n_streams], max_frames)]
 * and a pair with d_offsets[s + 1] <= d_offsets[s] is an empty stream. Ranges that overlap (offsets that decrease and rise again) give
 * undefined packets and records for the streams that overlap, and nothing worse.
 * STATE. One record per stream, an array of them, 16-byte aligned, in DEVICE memory for the _device entry. What stream s emits and
 * what its record holds afterwards equal, byte for byte, what one dvbs2_bbdeheader_t gives that is fed the same frames in the same
 * sequence of calls: the packets, the transport error indicators, the synchronised flag, the carried partial packet, the six counters
 * (the defined deviation `overruns` included). ALL-ZERO BYTES ARE THE BLOCK AS CONSTRUCTED: a hipMemsetAsync of one record resets that
 * stream, one of the array resets the batch; there is no init entry. A stream without frames in a call is not touched at all: its
 * record's bytes stay as they are. last_packets: the packets the stream wrote in the last call that touched it. `reserved` and the
 * padding are never read or written.
 *
 * Host only, no device needed:
 *   dvbs2_bbdeheader_rows_check     kbch_bits by the rules of dvbs2_bbdeheader_create_raw (>= 88, a multiple of 8, kbch_bits - 80 <= 65535,
 *                                   at most 64 packets per BBFRAME), n_streams 1..1024 (the limit of the gather that writes d_offsets),
 *                                   max_frames 1..2^20. DVBS2_EINVAL with a text that names the argument.
 *   dvbs2_bbdeheader_rows_geometry  kbch_bytes = kbch_bits / 8; max_out_bytes_per_frame as dvbs2_bbdeheader_params gives it; out_bytes =
 *                                   max_frames * max_out_bytes_per_frame, an upper bound whatever the headers say (a frame completes at
 *                                   most ceil(max DFL bytes / 188) packets: floor((187 + x) / 188) = ceil(x / 188)); work_bytes = the
 *                                   scratch of a call (per frame a header word, a plan and the stream it belongs to; per stream a tail
 *                                   plan). Every output nullable.
 *   dvbs2_bbdeheader_state_counters HOST copies of n_streams records as n_streams dvbs2_bbdeheader_counters_t.
 *
 * DEVICE entry, asynchronous on `stream` (a hipStream_t) of `device`; no allocation, no host synchronisation, FIVE launches for any
 * n_streams. The argument checks come first (the ranges above; no null pointer; d_offsets and d_pkt_offsets 4-byte aligned, d_state and
 * d_work 16-byte aligned: DVBS2_EINVAL; work_bytes and out_bytes at least the geometry's: DVBS2_ESIZE), the device is looked for after
 * them; a refused call writes nothing.
 *   dvbs2_bbdeheader_rows_device    188-byte packets, compact and stream-major, in d_ts_out. d_pkt_offsets (required, n_streams + 1
 *                                   entries) receives the exclusive prefix sums of the packets per stream: stream s owns the packets
 *                                   d_pkt_offsets[s] .. d_pkt_offsets[s + 1] of d_ts_out. It mirrors d_offsets, so the next consumer
 *                                   needs no host read either.
 * ORDER. Unlike the rotator rows, a call READS AND WRITES the records, and the workspace belongs to one call at a time: calls on the
 * same records or the same workspace must be ordered on one stream (or by events). d_ts_out and d_pkt_offsets are the call's own. */
typedef struct {
    int32_t synched, partial_ts_bytes;                          /* d_synched, d_partial_ts_bytes */
    uint64_t packets, errors, bbframes, dropped, gaps, overruns; /* as dvbs2_bbdeheader_counters_t */
    int32_t last_packets;
    int32_t reserved;
    uint8_t partial_pkt[188];                                   /* d_partial_pkt: its first partial_ts_bytes bytes count */
    uint8_t padding[4];                                         /* to 256 bytes */
} dvbs2_bbdeheader_state_t;
int dvbs2_bbdeheader_rows_check(int kbch_bits, int n_streams, int max_frames);
int dvbs2_bbdeheader_rows_geometry(int kbch_bits, int n_streams, int max_frames, int* kbch_bytes, int* max_out_bytes_per_frame,
                                   int64_t* work_bytes, int64_t* out_bytes);
int dvbs2_bbdeheader_state_counters(const dvbs2_bbdeheader_state_t* state, int n_streams, dvbs2_bbdeheader_counters_t* out);
int dvbs2_bbdeheader_rows_device(const uint8_t* d_bbframes, int kbch_bits, const int32_t* d_offsets, int n_streams, int max_frames,
                                 dvbs2_bbdeheader_state_t* d_state, void* d_work, int64_t work_bytes, uint8_t* d_ts_out, int64_t out_bytes,
                                 int32_t* d_pkt_offsets, int device, void* stream);

/* ---- BB framing: mode adaptation for MPEG-TS (EN 302 307-1 clauses 5.1.4 to 5.1.6), the mirror of dvbs2_bbdeheader_* above. In the
 * reference's transmit flowgraph the place is held by gr-dtv's dvb_bbheader_bb(..., INPUTMODE_NORMAL, ...) (apps/dvbs2-tx:619-621).
 * 188-byte TS packets in, BBFRAMEs of kbch_bytes out, every byte defined by the standard. Bytes only: nothing here has a tolerance.
 *
 * The handle is created for one kbch_bits: kbch_bytes = kbch_bits / 8, max_dfl_bytes = kbch_bytes - 10. It holds a position pos, the
 * number of bytes of the CRC-encoded stream E consumed since create or reset. E is defined over the packets P[0], P[1], ... presented
 * since then:
 *   E[188 p + i] = P[p][i] for i = 1..187
 *   E[188 p]     = for p >= 1 the CRC-8 of P[p - 1][1..187] (generator x^8 + x^7 + x^6 + x^4 + x^2 + 1, zero start, no reflection:
 *                  the byte that makes check_crc8(packet, 188) of lib/bbdeheader_bb_impl.cc:138-142 pass)
 *   E[0]         = P[0][0] unchanged (the receiver skips that byte when it synchronises)
 * A call (n_frames, dfl_bytes) writes n_frames BBFRAMEs of kbch_bytes each, back to back. Frame f has s = pos + f * dfl_bytes and holds
 *   bytes 0..9                  BBHEADER: MATYPE-1, MATYPE-2, UPL = 1504, DFL = 8 * dfl_bytes, SYNC = 0x47,
 *                               SYNCD = 8 * ((188 - s mod 188) mod 188), then the CRC-8 of those nine bytes
 *   bytes 10..10 + dfl_bytes-1  E[s .. s + dfl_bytes)
 *   the rest, up to kbch_bytes  zero padding
 * After the call pos += n_frames * dfl_bytes. dfl_bytes = 0 means max_dfl_bytes (packets straddle frames, as gr-dtv sends them);
 * otherwise it lies in 188..max_dfl_bytes, so every DATAFIELD holds a packet start and SYNCD never needs the 0xFFFF case.
 * (max_dfl_bytes / 188) * 188 gives whole packets per frame with padding; a short value on the last call flushes a stream; dfl_bytes may
 * change from call to call.
 * Packets a call reads: already presented P0 = ceil(pos / 188), needed up to P1 = ceil((pos + n_frames * dfl_bytes) / 188); the call
 * reads exactly P1 - P0 whole 188-byte packets from its input, P[P0] .. P[P1 - 1]. The handle carries between calls on the device the
 * unconsumed tail of a partly consumed packet (at most 187 bytes) and the CRC of the last packet presented. pos itself is arithmetic on
 * the call arguments; the handle mirrors it on the host, advanced only when a call was launched, so dvbs2_bbframer_need answers
 * without a synchronisation.
 * A presented packet whose byte 0 is not 0x47 is framed all the same (for p >= 1 the byte is replaced anyway) and counted in
 * sync_errors.
 * Refusals, each with a text that names the argument: kbch_bits as the de-header's (>= 88, a multiple of 8, kbch_bits - 80 <= 65535)
 * and max_dfl_bytes >= 188; max_frames in 1..65535; dfl_bytes 0 or in 188..max_dfl_bytes, otherwise DVBS2_EINVAL; matype bytes in
 * 0..255; n_frames < 0 or n_frames > max_frames is DVBS2_ESIZE; input and output ranges of a call that overlap are DVBS2_EINVAL.
 * n_frames == 0 is a valid call that changes nothing. */
typedef struct dvbs2_bbframer dvbs2_bbframer_t;
typedef struct { uint64_t packets, bbframes, sync_errors; } dvbs2_bbframer_counters_t;
int dvbs2_bbframer_create(dvbs2_bbframer_t** h, int standard, int framesize, int rate, int max_frames, int device);
int dvbs2_bbframer_create_raw(dvbs2_bbframer_t** h, int kbch_bits, int max_frames, int device);
void dvbs2_bbframer_destroy(dvbs2_bbframer_t* h);
int dvbs2_bbframer_params(const dvbs2_bbframer_t* h, int* kbch_bytes, int* max_dfl_bytes, int* max_packets_per_call);
/* default 0xF2, 0 (TS, SIS, CCM, roll-off 0.20); applies to later calls */
int dvbs2_bbframer_set_matype(dvbs2_bbframer_t* h, int matype1, int matype2);
/* host only: P1 - P0 for the NEXT call */
int dvbs2_bbframer_need(const dvbs2_bbframer_t* h, int n_frames, int dfl_bytes, int* n_packets);
/* device pointers, asynchronous on `stream`: no allocation, no host synchronisation, one launch. Calls on one handle are ordered by
 * the caller, as for dvbs2_enc_encode_device; the output is exactly what dvbs2_enc_encode_device takes as d_in for the same row (the
 * BB scrambler stays where it is: dvbs2_enc_set_scramble). */
int dvbs2_bbframer_process_device(dvbs2_bbframer_t* h, const uint8_t* d_ts, int n_frames, int dfl_bytes, uint8_t* d_bbframes, void* stream);
/* host pointers, synchronous, staged through the handle; *n_packets_read = packets taken from ts */
int dvbs2_bbframer_process(dvbs2_bbframer_t* h, const uint8_t* ts, int n_frames, int dfl_bytes, uint8_t* bbframes, int* n_packets_read);
/* synchronises `stream` */
int dvbs2_bbframer_counters(dvbs2_bbframer_t* h, dvbs2_bbframer_counters_t* out, void* stream);
/* pos 0, nothing carried, counters zero */
int dvbs2_bbframer_reset(dvbs2_bbframer_t* h, void* stream);
/* host only, no device: ten BBHEADER bytes with their CRC-8; the check byte of a string (remainder of data * x^8), or DVBS2_EINVAL */
int dvbs2_bbheader_build(uint8_t out[10], int matype1, int matype2, int upl_bits, int dfl_bits, int sync, int syncd_bits);
int dvbs2_crc8(const uint8_t* data, size_t n);

/*
 * ---- the batched stages: the part of the C ABI of libdvbs2_fec_hip.so that takes a BATCH of symbol streams from the symbol
 * synchroniser's output to the FEC chain's input: PLFRAME search, gather, coarse frequency estimate and front end for S streams in
 * a fixed number of launches. The conventions (return codes, dvbs2_last_error, DEVICE pointers and a hipStream_t as void* in the
 * "_device" entries, the answer to a null handle) are the ones stated at the top of this file.
 *
 * The arithmetic is that of the single-stream handles (dvbs2_plsync_*, dvbs2_plcoarse_*, dvbs2_plframe_*), and the device code is
 * shared with them: for every stream, every result here is, bit for bit, what a single-stream handle of its own gives for that
 * stream. The single-stream handles are the specification of this section, and its tests compare against them.
 *
 * The path for S streams, every step asynchronous on one stream, with ONE host wait (dvbs2_plsync_batch_finish, needed only to
 * learn each stream's `consumed`):
 *   dvbs2_symsync_work_device            S rows of symbols (existing)
 *   dvbs2_plsync_batch_search_device     records of every stream                          1 copy of 8 S bytes, 2 launches
 *   dvbs2_plsync_batch_gather_device     slots of plframe_len + 90 symbols, d_offsets     2 launches
 *   dvbs2_plcoarse_batch_estimate_device per-slot coarse_foffset / coarse_corrected        2 launches
 *   dvbs2_plframe_process_strided_device XFECFRAMEs of all slots of all streams            2 launches
 *   dvbs2_chain_*                        one FEC call over all frames (existing)
 */

/* ---- batched PLFRAME search. One handle holds max_streams independent trackers, each with the state of a dvbs2_plsync_t: machine
 * state, frame length, unlock count, absolute offset, resume point and the 89 symbols before its consumed point. plsc_or_minus1,
 * unlock_thresh, max_symbols (per stream) and max_frames (per stream) are as for dvbs2_plsync_create; max_streams is 1..1024.
 * set_plsc_mode and set_expected_pls act on the whole handle. dvbs2_plsync_batch_reset gives every stream as created,
 * dvbs2_plsync_batch_reset_stream one stream; both wait for the device.
 *
 * dvbs2_plsync_batch_search_device: stream s reads n_syms[s] symbols from d_syms + 2 * (s * stride_syms + first[s]) floats. first and
 * n_syms are HOST arrays of n_streams ints; the call takes its copy of them before it returns, as dvbs2_symsync_work_device does with
 * n_in. first[s] lets every stream be presented again from its own `consumed` without a copy. n_syms[s] == 0 is legal and leaves
 * stream s untouched: it reports no frame, consumes nothing, and its state is the one it had. With more than one stream a row must
 * not run into the next (first[s] + n_syms[s] <= stride_syms). d_syms must be 8-byte aligned. d_frames is [n_streams][max_frames]
 * records of dvbs2_plsync_frame_t, stream s's at d_frames + s * max_frames. Two launches for any number of streams: the timing metric
 * over a (tile, stream) grid, then one wavefront per stream. dvbs2_plsync_batch_finish waits for the last search and fills arrays of
 * that search's n_streams ints (each nullable): one wait, one copy.
 *
 * dvbs2_plsync_batch_gather_device refers to the buffers of the LAST search, including that search's first[] (d_syms and stride_syms
 * are passed again, as dvbs2_plsync_gather_device takes d_syms again); n_streams is at most that search's. Every reported frame that
 * is locked and carries wanted_plsc is copied into a SLOT of plframe_len + 90 symbols: the frame and the 90 symbols that follow it in
 * its own stream (the buffer-end rule guarantees they lie inside the buffer). Slots are stream-major and in stream order within a
 * stream. d_offsets[0 .. n_streams] (int32) receives the prefix sums of the selected counts: stream s owns slots d_offsets[s] ..
 * d_offsets[s + 1]. These are the true counts even above max_slots; slots with index >= max_slots are not written. d_slot_record is
 * nullable; when given, slot i receives its (stream, record index) as two int32. d_slots should be 16-byte aligned. Every slot
 * carries its own next header, so slots of any streams can share one dvbs2_plframe_*_strided_device launch, and a pilotless front
 * end sees the true next header also when other frames lie between two gathered ones.
 *
 * dvbs2_plsync_batch_check (host only) holds the argument ranges of create; dvbs2_plsync_batch_check_search (host only) those of a
 * search against a handle's max_streams and max_symbols: the two entries call them first. */
typedef struct dvbs2_plsync_batch dvbs2_plsync_batch_t;
int dvbs2_plsync_batch_check(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames);
int dvbs2_plsync_batch_check_search(int max_streams, int max_symbols, int64_t stride_syms, const int* first, const int* n_syms, int n_streams);
int dvbs2_plsync_batch_create(dvbs2_plsync_batch_t** h, int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames,
                              int device);
void dvbs2_plsync_batch_destroy(dvbs2_plsync_batch_t* h);
int dvbs2_plsync_batch_reset(dvbs2_plsync_batch_t* h);
int dvbs2_plsync_batch_reset_stream(dvbs2_plsync_batch_t* h, int stream_index);
int dvbs2_plsync_batch_set_plsc_mode(dvbs2_plsync_batch_t* h, int coherent, int soft);
int dvbs2_plsync_batch_set_expected_pls(dvbs2_plsync_batch_t* h, const uint8_t* plsc_list, int n);
int dvbs2_plsync_batch_search_device(dvbs2_plsync_batch_t* h, const float* d_syms, int64_t stride_syms, const int* first, const int* n_syms,
                                     int n_streams, dvbs2_plsync_frame_t* d_frames, void* stream);
int dvbs2_plsync_batch_finish(dvbs2_plsync_batch_t* h, int* n_frames, int* consumed, int* state);
int dvbs2_plsync_batch_gather_device(dvbs2_plsync_batch_t* h, const float* d_syms, int64_t stride_syms, const dvbs2_plsync_frame_t* d_frames,
                                     int n_streams, int wanted_plsc, float* d_slots, int max_slots, int32_t* d_offsets, int32_t* d_slot_record,
                                     void* stream);

/* ---- strided PLFRAME front end: dvbs2_plframe_estimate_device / dvbs2_plframe_process_device with frame f at symbol f * stride_syms
 * of d_slots and its next header inside its slot, stride_syms >= plframe_len + 90 (dvbs2_plframe_stride_check, host only, holds the
 * rule). Every frame has a next header, so there is no has_trailing_header. The back-to-back entries are this with stride
 * plframe_len and keep their bits. */
int dvbs2_plframe_stride_check(int plsc, int64_t stride_syms);
int dvbs2_plframe_estimate_strided_device(dvbs2_plframe_t* h, const float* d_slots, int64_t stride_syms, int n_frames,
                                          const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                                          const dvbs2_plframe_estimates_t* d_est, void* stream);
int dvbs2_plframe_process_strided_device(dvbs2_plframe_t* h, const float* d_slots, int64_t stride_syms, int n_frames,
                                         const int32_t* d_coarse_corrected, const float* d_coarse_foffset, float* d_xfecframes,
                                         const dvbs2_plframe_estimates_t* d_est, void* stream);

/* ---- batched coarse frequency estimate: dvbs2_plcoarse_estimate_device over the slots of a gather, with one window state per
 * stream. period and plsc_or_minus1 as for dvbs2_plcoarse_create; max_streams 1..1024; max_slots 1..1048576. The autocorrelation
 * runs over max_slots wavefronts, of which those at or beyond d_offsets[n_streams] leave at once; then one wavefront per stream walks
 * slots d_offsets[s] .. d_offsets[s + 1] (those below max_slots) in order over its own state. d_offsets is read on the DEVICE: no host
 * round trip lies between gather and estimate. d_plsc: one byte per slot, or NULL for the handle's fixed PLSC. The outputs are per
 * slot, each nullable: exactly the arrays dvbs2_plframe_*_strided_device reads. A stream without a slot in a call keeps its state.
 * d_slots and the outputs must have room for min(d_offsets[n_streams], max_slots) slots: give the gather the handle's max_slots, or less.
 * dvbs2_plcoarse_batch_reset / _reset_stream wait for the device. */
typedef struct dvbs2_plcoarse_batch dvbs2_plcoarse_batch_t;
int dvbs2_plcoarse_batch_create(dvbs2_plcoarse_batch_t** h, int period, int plsc_or_minus1, int max_streams, int max_slots, int device);
void dvbs2_plcoarse_batch_destroy(dvbs2_plcoarse_batch_t* h);
int dvbs2_plcoarse_batch_reset(dvbs2_plcoarse_batch_t* h);
int dvbs2_plcoarse_batch_reset_stream(dvbs2_plcoarse_batch_t* h, int stream_index);
int dvbs2_plcoarse_batch_estimate_device(dvbs2_plcoarse_batch_t* h, const float* d_slots, int64_t stride_syms, const uint8_t* d_plsc,
                                         const int32_t* d_offsets, int n_streams, float* d_coarse_foffset, int32_t* d_coarse_corrected,
                                         int32_t* d_new_est, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DVBS2_FEC_HIP_H */
