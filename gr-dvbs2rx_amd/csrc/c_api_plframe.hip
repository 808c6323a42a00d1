// c_api_plframe.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the PLFRAME front end.
#include "c_api_common.h"
#include "plframe_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ PLFRAME front end: PLSC, phases, fine offset */
struct dvbs2_plframe {
    PlFrameHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, CF, CC, EST, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // EST: sof | plheader | fine | pilot phases | fine_valid (int32) | plsc (uint8)
    int device = 0;
};

static int plframe_check(const dvbs2_plframe* h, const void* plframes, int n_frames, const void* cc, const void* cf)
{
    NEED_HANDLE(h);
    if (n_frames < 0 || (n_frames && (!plframes || !cc))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames && h->impl->pls().n_pilots == 0 && !cf) return fail(DVBS2_EINVAL, "a pilotless handle needs coarse_foffset");
    if (n_frames > h->impl->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

static PlFrameEstimates plframe_est(const dvbs2_plframe_estimates_t* e)
{
    PlFrameEstimates o;
    if (e) { o.plsc_decoded = e->plsc_decoded; o.sof_phase = e->sof_phase; o.plheader_phase = e->plheader_phase;
             o.pilot_phase = e->pilot_phase; o.fine_foffset = e->fine_foffset; o.fine_valid = e->fine_valid; }
    return o;
}

// host entry: stage in, run, copy back what the caller asked for
static int plframe_host(dvbs2_plframe* h, const float* plframes, int n_frames, int trailing, const int32_t* cc, const float* cf,
                        float* xfecframes, const dvbs2_plframe_estimates_t* est)
{
    if (int rc = plframe_check(h, plframes, n_frames, cc, cf)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const PlsInfo& p = h->impl->pls();
    const size_t mf = h->impl->max_frames(), fl = p.plframe_len, xl = p.xfecframe_len, nf = n_frames, np = p.n_pilots;
    if (s.ensure(h->IN, (mf * fl + 90) * 8) || s.ensure(h->OUT, mf * xl * 8) || s.ensure(h->CF, mf * 4) || s.ensure(h->CC, mf * 4) ||
        s.ensure(h->EST, mf * (4 + (np ? np : 1)) * 4 + mf)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT); float* d_cf = s.at<float>(h->CF); int32_t* d_cc = s.at<int32_t>(h->CC);
    float* d_est = s.at<float>(h->EST);
    PlFrameEstimates d;
    d.sof_phase = d_est; d.plheader_phase = d_est + mf; d.fine_foffset = d_est + 2 * mf; d.pilot_phase = d_est + 3 * mf;
    d.fine_valid = reinterpret_cast<int32_t*>(d_est + (3 + (np ? np : 1)) * mf);
    d.plsc_decoded = reinterpret_cast<uint8_t*>(d_est + (4 + (np ? np : 1)) * mf);
    HCHK(hipMemcpyAsync(d_in, plframes, (nf * fl + (trailing ? 90 : 0)) * 8, hipMemcpyHostToDevice, s.stream));
    HCHK(hipMemcpyAsync(d_cc, cc, nf * 4, hipMemcpyHostToDevice, s.stream));
    if (cf) HCHK(hipMemcpyAsync(d_cf, cf, nf * 4, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->run_device(d_in, n_frames, trailing, d_cc, cf ? d_cf : nullptr, xfecframes ? d_out : nullptr, d, s.stream))) return rc;
    if (xfecframes) HCHK(hipMemcpyAsync(xfecframes, d_out, nf * xl * 8, hipMemcpyDeviceToHost, s.stream));
    if (est) {
        if (est->sof_phase) HCHK(hipMemcpyAsync(est->sof_phase, d.sof_phase, nf * 4, hipMemcpyDeviceToHost, s.stream));
        if (est->plheader_phase) HCHK(hipMemcpyAsync(est->plheader_phase, d.plheader_phase, nf * 4, hipMemcpyDeviceToHost, s.stream));
        if (est->fine_foffset) HCHK(hipMemcpyAsync(est->fine_foffset, d.fine_foffset, nf * 4, hipMemcpyDeviceToHost, s.stream));
        if (est->pilot_phase && np) HCHK(hipMemcpyAsync(est->pilot_phase, d.pilot_phase, nf * np * 4, hipMemcpyDeviceToHost, s.stream));
        if (est->fine_valid) HCHK(hipMemcpyAsync(est->fine_valid, d.fine_valid, nf * 4, hipMemcpyDeviceToHost, s.stream));
        if (est->plsc_decoded) HCHK(hipMemcpyAsync(est->plsc_decoded, d.plsc_decoded, nf, hipMemcpyDeviceToHost, s.stream));
    }
    return s.sync();
}

extern "C" {

int dvbs2_plheader_symbols(int plsc, float* syms90)
{
    if (!syms90 || plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "bad argument");
    plheader_symbols(plsc, syms90);
    return DVBS2_OK;
}

int dvbs2_pls_parse(int plsc, int* plframe_len, int* payload_len, int* xfecframe_len, int* n_slots, int* n_pilots, int* n_mod)
{
    if (plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    const PlsInfo p = pls_parse(plsc);
    if (plframe_len) *plframe_len = p.plframe_len;
    if (payload_len) *payload_len = p.payload_len;
    if (xfecframe_len) *xfecframe_len = p.xfecframe_len;
    if (n_slots) *n_slots = p.n_slots;
    if (n_pilots) *n_pilots = p.n_pilots;
    if (n_mod) *n_mod = p.n_mod;
    return DVBS2_OK;
}

int dvbs2_plframe_create(dvbs2_plframe_t** h, int gold_code, int plsc, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad PLSC is the caller's mistake on any machine
    if (plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    { const PlsInfo p = pls_parse(plsc); if (p.n_mod == 0 && !p.dummy_frame) return fail(DVBS2_EINVAL, "plsc names a reserved MODCOD (29..31)"); }
    if (gold_code < 0 || gold_code >= (1 << 18) - 1) return fail(DVBS2_EINVAL, "gold code out of range");
    return make_handle(h, device, [&] { return new (std::nothrow) PlFrameHip(gold_code, plsc, max_frames, device); });
    API_CATCH
}

void dvbs2_plframe_destroy(dvbs2_plframe_t* h) { destroy_handle(h); }

int dvbs2_plframe_params(const dvbs2_plframe_t* h, int* plframe_len, int* payload_len, int* xfecframe_len, int* n_slots, int* n_pilots,
                         int* n_mod)
{
    NEED_HANDLE(h);
    return dvbs2_pls_parse(h->impl->pls().plsc, plframe_len, payload_len, xfecframe_len, n_slots, n_pilots, n_mod);
}

int dvbs2_plframe_set_plsc_mode(dvbs2_plframe_t* h, int coherent, int soft)
{
    NEED_HANDLE(h);
    h->impl->set_plsc_mode(coherent, soft);
    return DVBS2_OK;
}

int dvbs2_plframe_set_expected_pls(dvbs2_plframe_t* h, const uint8_t* plsc_list, int n)
{
    API_TRY
    NEED_HANDLE(h);
    if (n < 0 || (n > 0 && !plsc_list)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->set_expected_pls(plsc_list, n));
    API_CATCH
}

int dvbs2_plframe_estimate_device(dvbs2_plframe_t* h, const float* d_plframes, int n_frames, int has_trailing_header,
                                  const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                                  const dvbs2_plframe_estimates_t* d_est, void* stream)
{
    API_TRY
    if (int rc = plframe_check(h, d_plframes, n_frames, d_coarse_corrected, d_coarse_foffset)) return rc;
    return impl_rc(h, h->impl->run_device(d_plframes, n_frames, has_trailing_header, d_coarse_corrected, d_coarse_foffset, nullptr, plframe_est(d_est),
                                          (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plframe_process_device(dvbs2_plframe_t* h, const float* d_plframes, int n_frames, int has_trailing_header,
                                 const int32_t* d_coarse_corrected, const float* d_coarse_foffset, float* d_xfecframes,
                                 const dvbs2_plframe_estimates_t* d_est, void* stream)
{
    API_TRY
    if (int rc = plframe_check(h, d_plframes, n_frames, d_coarse_corrected, d_coarse_foffset)) return rc;
    if (n_frames && !d_xfecframes) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->run_device(d_plframes, n_frames, has_trailing_header, d_coarse_corrected, d_coarse_foffset, d_xfecframes, plframe_est(d_est),
                                          (hipStream_t)stream));
    API_CATCH
}

/* ---- one slot per frame (what dvbs2_plsync_batch_gather_device writes): frame f at f * stride_syms with its next header behind it */
int dvbs2_plframe_stride_check(int plsc, int64_t stride_syms)
{
    if (plsc < 0 || plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    if (stride_syms < (int64_t)pl_frame_shape(plsc).plframe_len + 90) return fail(DVBS2_EINVAL, "stride_syms below plframe_len + 90");
    if (stride_syms > INT32_MAX) return fail(DVBS2_EINVAL, "stride_syms above 2^31 - 1");
    return DVBS2_OK;
}

int dvbs2_plframe_estimate_strided_device(dvbs2_plframe_t* h, const float* d_slots, int64_t stride_syms, int n_frames,
                                          const int32_t* d_coarse_corrected, const float* d_coarse_foffset,
                                          const dvbs2_plframe_estimates_t* d_est, void* stream)
{
    API_TRY
    if (int rc = plframe_check(h, d_slots, n_frames, d_coarse_corrected, d_coarse_foffset)) return rc;
    if (int rc = dvbs2_plframe_stride_check(h->impl->pls().plsc, stride_syms)) return rc;
    return impl_rc(h, h->impl->run_strided_device(d_slots, (int)stride_syms, n_frames, d_coarse_corrected, d_coarse_foffset, nullptr, plframe_est(d_est),
                                                  (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plframe_process_strided_device(dvbs2_plframe_t* h, const float* d_slots, int64_t stride_syms, int n_frames,
                                         const int32_t* d_coarse_corrected, const float* d_coarse_foffset, float* d_xfecframes,
                                         const dvbs2_plframe_estimates_t* d_est, void* stream)
{
    API_TRY
    if (int rc = plframe_check(h, d_slots, n_frames, d_coarse_corrected, d_coarse_foffset)) return rc;
    if (int rc = dvbs2_plframe_stride_check(h->impl->pls().plsc, stride_syms)) return rc;
    if (n_frames && !d_xfecframes) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->run_strided_device(d_slots, (int)stride_syms, n_frames, d_coarse_corrected, d_coarse_foffset, d_xfecframes,
                                                  plframe_est(d_est), (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plframe_estimate(dvbs2_plframe_t* h, const float* plframes, int n_frames, int has_trailing_header,
                           const int32_t* coarse_corrected, const float* coarse_foffset, const dvbs2_plframe_estimates_t* est)
{
    API_TRY
    return plframe_host(h, plframes, n_frames, has_trailing_header, coarse_corrected, coarse_foffset, nullptr, est);
    API_CATCH
}

int dvbs2_plframe_process(dvbs2_plframe_t* h, const float* plframes, int n_frames, int has_trailing_header,
                          const int32_t* coarse_corrected, const float* coarse_foffset, float* xfecframes,
                          const dvbs2_plframe_estimates_t* est)
{
    API_TRY
    if (n_frames > 0 && !xfecframes) return fail(DVBS2_EINVAL, "bad argument");
    return plframe_host(h, plframes, n_frames, has_trailing_header, coarse_corrected, coarse_foffset, xfecframes, est);
    API_CATCH
}

} // extern "C"
