// c_api_fec.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the BCH decoder and the demapper handles.
#include "c_api_fec.h"
#include "fec_tables.h"
#include "demap_math.hpp"

using namespace dvbs2;

/* ------------------------------------------------------------------ BCH */
static int bch_make(dvbs2_bch_t** h, int m, uint32_t prim_poly, int t, int n, int max_frames, int device)
{
    return make_handle(h, device, [&] { return new (std::nothrow) BchDecoderHip(m, prim_poly, t, n, max_frames, device); });
}

static void bch_field(int framesize, int* m, uint32_t* prim)
{   // reference lib/bch_decoder_bb_impl.cc:58-63
    if (framesize == DVBS2_FECFRAME_NORMAL) { *m = 16; *prim = 0x1002Du; }      // x^16 + x^5 + x^3 + x^2 + 1
    else if (framesize == DVBS2_FECFRAME_SHORT) { *m = 14; *prim = 0x402Bu; }   // x^14 + x^5 + x^3 + x + 1
    else { *m = 15; *prim = 0x802Du; }                                           // x^15 + x^5 + x^3 + x^2 + 1
}

extern "C" {

int dvbs2_bch_create(dvbs2_bch_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    int m; uint32_t prim;
    bch_field(framesize, &m, &prim);
    int rc = bch_make(h, m, prim, (int)fi.bch_t, (int)fi.bch_n, max_frames, device);
    if (rc == DVBS2_OK && (*h)->impl->code().k != (int)fi.bch_k) { dvbs2_bch_destroy(*h); *h = nullptr; return fail(DVBS2_EINVAL, "BCH k mismatch with the parameter table"); }
    return rc;
    API_CATCH
}

int dvbs2_bch_create_raw(dvbs2_bch_t** h, int m, uint32_t prim_poly, int t, int n, int max_frames, int device)
{
    API_TRY
    return bch_make(h, m, prim_poly, t, n, max_frames, device);
    API_CATCH
}

void dvbs2_bch_destroy(dvbs2_bch_t* h) { destroy_handle(h); }

int dvbs2_bch_params(const dvbs2_bch_t* h, int* n, int* k, int* t)
{
    NEED_HANDLE(h);
    if (n) *n = h->impl->code().n; if (k) *k = h->impl->code().k; if (t) *t = h->impl->code().t;
    return DVBS2_OK;
}

int dvbs2_bch_genpoly(const dvbs2_bch_t* h, uint8_t* gen, int max_coefs)
{
    NEED_HANDLE(h);
    const auto& g = h->impl->code().gen;
    if (gen) for (int i = 0; i < (int)g.size() && i < max_coefs; i++) gen[i] = g[i];
    return h->impl->code().gdeg;
}

int dvbs2_bch_set_descramble(dvbs2_bch_t* h, int enable)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_descramble(enable != 0));
    API_CATCH
}

int dvbs2_bb_descramble_sequence(uint8_t* seq, int n_bytes)
{
    if (!seq || n_bytes < 0 || n_bytes > 64800 / 8) return fail(DVBS2_EINVAL, "bad argument");
    bb_derandomise_sequence(seq, n_bytes);
    return DVBS2_OK;
}

int dvbs2_bch_decode_device(dvbs2_bch_t* h, const uint8_t* d_cw, int n_frames, uint8_t* d_msg, int32_t* d_corr, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_cw && d_msg && d_corr)) return rc;
    return impl_rc(h, h->impl->decode_device(d_cw, n_frames, d_msg, d_corr, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_bch_decode(dvbs2_bch_t* h, const uint8_t* cw, int n_frames, uint8_t* msg, int32_t* corrections)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, cw && msg && corrections)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t nb = h->impl->code().n / 8, kb = h->impl->code().k / 8, mf = h->impl->max_frames();
    if (s.ensure(h->CW, mf * nb) || s.ensure(h->MSG, mf * kb) || s.ensure(h->CORR, mf * 4)) return DVBS2_EDEVICE;
    uint8_t* d_cw = s.at<uint8_t>(h->CW); uint8_t* d_msg = s.at<uint8_t>(h->MSG); int32_t* d_corr = s.at<int32_t>(h->CORR);
    HCHK(hipMemcpyAsync(d_cw, cw, (size_t)n_frames * nb, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->decode_device(d_cw, n_frames, d_msg, d_corr, s.stream))) return rc;
    HCHK(hipMemcpyAsync(msg, d_msg, (size_t)n_frames * kb, hipMemcpyDeviceToHost, s.stream));
    HCHK(hipMemcpyAsync(corrections, d_corr, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

/* ------------------------------------------------------------------ demapper */
int dvbs2_demap_create(dvbs2_demap_t** h, int framesize, int rate, int constellation, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, [&] { return new (std::nothrow) DemapperHip(framesize, rate, constellation, max_frames, device); });
    API_CATCH
}

int dvbs2_demap_table_check(int n_mod, const float* points_re_im, const uint8_t* column)
{
    API_TRY
    std::string why;
    return demap_table_check(n_mod, points_re_im, column, &why) ? DVBS2_OK : fail(DVBS2_EINVAL, why);
    API_CATCH
}

int dvbs2_demap_create_table(dvbs2_demap_t** h, int framesize, int n_mod, const float* points_re_im, const uint8_t* column, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    if (int rc = dvbs2_demap_table_check(n_mod, points_re_im, column)) return rc; // before any device is touched
    return make_handle(h, device, [&] { return new (std::nothrow) DemapperHip(framesize, n_mod, points_re_im, column, max_frames, device); });
    API_CATCH
}

int dvbs2_demap_table(const dvbs2_demap_t* h, int* n_mod, float* points_re_im, uint8_t* column)
{
    NEED_HANDLE(h);
    if (!h->impl->is_table()) return fail(DVBS2_EINVAL, "not a table handle (dvbs2_demap_create_table)");
    h->impl->table(n_mod, points_re_im, column);
    return DVBS2_OK;
}

void dvbs2_demap_destroy(dvbs2_demap_t* h) { destroy_handle(h); }

int dvbs2_apsk_points(int constellation, int rate, float* re_im)
{
    if (!re_im) return fail(DVBS2_EINVAL, "bad argument");
    if (constellation != DVBS2_MOD_16APSK && constellation != DVBS2_MOD_32APSK) return fail(DVBS2_EINVAL, "Unsupported constellation");
    if (!apsk_points(constellation, rate, re_im)) return fail(DVBS2_EINVAL, "Unsupported code rate for 16APSK / 32APSK");
    return DVBS2_OK;
}

int dvbs2_demap_params(const dvbs2_demap_t* h, int* n_syms, int* n_llr, int* n_mod, int* column_order)
{
    NEED_HANDLE(h);
    if (n_syms) *n_syms = h->impl->n_syms(); if (n_llr) *n_llr = h->impl->n_llr();
    if (n_mod) *n_mod = h->impl->n_mod(); if (column_order) *column_order = h->impl->column_order();
    return DVBS2_OK;
}

int dvbs2_demap_soft_device(dvbs2_demap_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count, int8_t* d_llr_out, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_syms && d_n0 && d_llr_out, n0_count != 1 && n0_count != n_frames)) return rc;
    return impl_rc(h, h->impl->soft_device(d_syms, n_frames, d_n0, n0_count, d_llr_out, (hipStream_t)stream));
    API_CATCH
}

// what the three host entries of the demapper share after their checks: every staging buffer there, the symbols on their way to the device
static int demap_stage(dvbs2_demap_t* h, const float* syms, int n_frames)
{
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = h->impl->max_frames(), ns = h->impl->n_syms();
    if (s.ensure(h->SYMS, mf * ns * 8) || s.ensure(h->N0, mf * 4) || s.ensure(h->LLR, mf * h->impl->n_llr()) || s.ensure(h->SNR, mf * 4)) return DVBS2_EDEVICE;
    HCHK(hipMemcpyAsync(s.buf[h->SYMS], syms, (size_t)n_frames * ns * 8, hipMemcpyHostToDevice, s.stream));
    return DVBS2_OK;
}

int dvbs2_demap_soft(dvbs2_demap_t* h, const float* syms, int n_frames, const float* n0, int n0_count, int8_t* llr_out)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, syms && n0 && llr_out, n0_count != 1 && n0_count != n_frames)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    if (int rc = demap_stage(h, syms, n_frames)) return rc;
    HostStage& s = h->stage;
    float* d_syms = s.at<float>(h->SYMS); float* d_n0 = s.at<float>(h->N0); int8_t* d_llr = s.at<int8_t>(h->LLR);
    HCHK(hipMemcpyAsync(d_n0, n0, (size_t)n0_count * 4, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->soft_device(d_syms, n_frames, d_n0, n0_count, d_llr, s.stream))) return rc;
    HCHK(hipMemcpyAsync(llr_out, d_llr, (size_t)n_frames * h->impl->n_llr(), hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

int dvbs2_demap_estimate_snr_device(dvbs2_demap_t* h, const float* d_syms, int n_frames, float* d_snr_lin, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_syms && d_snr_lin)) return rc;
    return impl_rc(h, h->impl->snr_device(d_syms, nullptr, n_frames, d_snr_lin, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_demap_estimate_snr(dvbs2_demap_t* h, const float* syms, int n_frames, float* snr_lin)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, syms && snr_lin)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    if (int rc = demap_stage(h, syms, n_frames)) return rc;
    HostStage& s = h->stage;
    float* d_syms = s.at<float>(h->SYMS); float* d_snr = s.at<float>(h->SNR);
    if (int rc = impl_rc(h, h->impl->snr_device(d_syms, nullptr, n_frames, d_snr, s.stream))) return rc;
    HCHK(hipMemcpyAsync(snr_lin, d_snr, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

int dvbs2_demap_refine_snr_device(dvbs2_demap_t* h, const float* d_syms, const int8_t* d_ref_llr, int n_frames, float* d_snr_lin, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_syms && d_ref_llr && d_snr_lin)) return rc;
    return impl_rc(h, h->impl->snr_device(d_syms, d_ref_llr, n_frames, d_snr_lin, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_demap_refine_snr(dvbs2_demap_t* h, const float* syms, const int8_t* ref_llr, int n_frames, float* snr_lin)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, syms && ref_llr && snr_lin)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    if (int rc = demap_stage(h, syms, n_frames)) return rc;
    HostStage& s = h->stage;
    float* d_syms = s.at<float>(h->SYMS); int8_t* d_llr = s.at<int8_t>(h->LLR); float* d_snr = s.at<float>(h->SNR);
    HCHK(hipMemcpyAsync(d_llr, ref_llr, (size_t)n_frames * h->impl->n_llr(), hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->snr_device(d_syms, d_llr, n_frames, d_snr, s.stream))) return rc;
    HCHK(hipMemcpyAsync(snr_lin, d_snr, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
