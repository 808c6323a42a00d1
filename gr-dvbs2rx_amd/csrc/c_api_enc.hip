// c_api_enc.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the encoder handle (BB scrambler -> BCH -> LDPC -> mapper).
#include "c_api_common.h"
#include "enc_hip.h"

using namespace dvbs2;

struct dvbs2_enc {
    EncoderHip* impl = nullptr;
    HostStage stage; enum { IN, BCH, LDPC, SYMS, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

static int enc_make(dvbs2_enc_t** h, const EncSpec& spec, int max_frames, int device)
{
    return make_handle(h, device, [&] { return new (std::nothrow) EncoderHip(spec, max_frames, device); });
}

// the checks every encode entry makes before the stage class is asked (its own texts name the arguments)
static int enc_check_call(const dvbs2_enc_t* h, int n_frames)
{
    NEED_HANDLE(h);
    if (n_frames < 0) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames > h->impl->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_enc_check(int standard, int framesize, int rate, int constellation)
{
    API_TRY
    EncSpec spec; std::string why;
    return enc_spec(standard, framesize, rate, constellation == kEncCallerTable ? -3 : constellation, &spec, &why) ? DVBS2_OK : fail(DVBS2_EINVAL, why);
    API_CATCH
}

int dvbs2_enc_create(dvbs2_enc_t** h, int standard, int framesize, int rate, int constellation, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    EncSpec spec; std::string why;
    if (!enc_spec(standard, framesize, rate, constellation == kEncCallerTable ? -3 : constellation, &spec, &why)) return fail(DVBS2_EINVAL, why); // before any device is touched
    return enc_make(h, spec, max_frames, device);
    API_CATCH
}

int dvbs2_enc_create_table(dvbs2_enc_t** h, int standard, int framesize, int rate, int n_mod, const float* points_re_im,
                           const uint8_t* column, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    EncSpec spec; std::string why;
    if (!enc_spec(standard, framesize, rate, kEncCallerTable, &spec, &why)) return fail(DVBS2_EINVAL, why);
    if (!enc_table_mapper(spec.table->N, n_mod, points_re_im, column, &spec.map, &why)) return fail(DVBS2_EINVAL, why);
    return enc_make(h, spec, max_frames, device);
    API_CATCH
}

int dvbs2_enc_create_parts(dvbs2_enc_t** h, int bch_m, uint32_t bch_prim_poly, int bch_t, int bch_n, const char* ldpc_table,
                           int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    EncSpec spec;
    if (!bch_m && !ldpc_table) return fail(DVBS2_EINVAL, "at least one of the BCH and the LDPC stage is required");
    spec.bch_m = bch_m; spec.bch_prim = bch_prim_poly; spec.bch_t = bch_t; spec.bch_n = bch_n;
    if (ldpc_table && !(spec.table = find_ldpc_table(ldpc_table))) return fail(DVBS2_EINVAL, std::string("ldpc_table: unknown LDPC table ") + ldpc_table);
    return enc_make(h, spec, max_frames, device);
    API_CATCH
}

void dvbs2_enc_destroy(dvbs2_enc_t* h) { destroy_handle(h); }

int dvbs2_enc_params(const dvbs2_enc_t* h, int* in_bits, int* bch_n, int* ldpc_n, int* n_syms, int* n_mod)
{
    NEED_HANDLE(h);
    if (in_bits) *in_bits = h->impl->in_bits(); if (bch_n) *bch_n = h->impl->bch_n(); if (ldpc_n) *ldpc_n = h->impl->ldpc_n();
    if (n_syms) *n_syms = h->impl->n_syms(); if (n_mod) *n_mod = h->impl->n_mod();
    return DVBS2_OK;
}

int dvbs2_enc_set_scramble(dvbs2_enc_t* h, int enable)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_scramble(enable != 0));
    API_CATCH
}

int dvbs2_enc_encode_device(dvbs2_enc_t* h, const uint8_t* d_in, int n_frames, uint8_t* d_bch_cw, uint8_t* d_ldpc_cw, float* d_syms, void* stream)
{
    API_TRY
    if (int rc = enc_check_call(h, n_frames)) return rc;
    return impl_rc(h, h->impl->encode_device(d_in, n_frames, d_bch_cw, d_ldpc_cw, d_syms, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_enc_encode(dvbs2_enc_t* h, const uint8_t* in, int n_frames, uint8_t* bch_cw, uint8_t* ldpc_cw, float* syms)
{
    API_TRY
    if (int rc = enc_check_call(h, n_frames)) return rc;
    EncoderHip* e = h->impl;
    // the refusals that need no device come from the stage class, on pointers that stand for the caller's: a present output stays non-null
    if (n_frames == 0 || !in || (bch_cw && !e->bch_n()) || (ldpc_cw && !e->ldpc_n()) || (syms && !e->n_mod()) || (!bch_cw && !ldpc_cw && !syms))
        return impl_rc(h, e->encode_device(in, n_frames, bch_cw, ldpc_cw, syms, nullptr) != 0);
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = e->max_frames(), ib = e->in_bits() / 8, bb = e->bch_n() / 8, lb = e->ldpc_n() / 8, sb = (size_t)e->n_syms() * 8;
    if (s.ensure(h->IN, mf * ib) || (bch_cw && s.ensure(h->BCH, mf * bb)) || (ldpc_cw && s.ensure(h->LDPC, mf * lb)) || (syms && s.ensure(h->SYMS, mf * sb))) return DVBS2_EDEVICE;
    uint8_t* d_bch = bch_cw ? s.at<uint8_t>(h->BCH) : nullptr; uint8_t* d_ldpc = ldpc_cw ? s.at<uint8_t>(h->LDPC) : nullptr;
    float* d_syms = syms ? s.at<float>(h->SYMS) : nullptr;
    HCHK(hipMemcpyAsync(s.buf[h->IN], in, (size_t)n_frames * ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, e->encode_device(s.at<uint8_t>(h->IN), n_frames, d_bch, d_ldpc, d_syms, s.stream))) return rc;
    if (bch_cw) HCHK(hipMemcpyAsync(bch_cw, d_bch, (size_t)n_frames * bb, hipMemcpyDeviceToHost, s.stream));
    if (ldpc_cw) HCHK(hipMemcpyAsync(ldpc_cw, d_ldpc, (size_t)n_frames * lb, hipMemcpyDeviceToHost, s.stream));
    if (syms) HCHK(hipMemcpyAsync(syms, d_syms, (size_t)n_frames * sb, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
