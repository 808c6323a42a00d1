// c_api_plpayload.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the PLFRAME payload step.
#include "c_api_common.h"
#include "plpayload_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ PLFRAME payload step */
struct dvbs2_plpayload {
    PlPayloadHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, PAR, CC, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

extern "C" {

int dvbs2_pl_scrambling_rn(int gold_code, uint8_t* rn, int n)
{
    API_TRY
    if (!rn || n < 0 || n > 360 * 90 + 22 * 36 || gold_code < 0 || gold_code >= (1 << 18) - 1) return fail(DVBS2_EINVAL, "bad argument");
    pl_scrambling_rn(gold_code, rn, n);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plpayload_create(dvbs2_plpayload_t** h, int gold_code, int n_slots, int has_pilots, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, [&] { return new (std::nothrow) PlPayloadHip(gold_code, n_slots, has_pilots, max_frames, device); });
    API_CATCH
}

void dvbs2_plpayload_destroy(dvbs2_plpayload_t* h) { destroy_handle(h); }

int dvbs2_plpayload_params(const dvbs2_plpayload_t* h, int* payload_len, int* xfecframe_len, int* n_pilots)
{
    NEED_HANDLE(h);
    if (payload_len) *payload_len = h->impl->payload_len();
    if (xfecframe_len) *xfecframe_len = h->impl->xfecframe_len();
    if (n_pilots) *n_pilots = h->impl->n_pilots();
    return DVBS2_OK;
}

int dvbs2_plpayload_process_device(dvbs2_plpayload_t* h, const float* d_payload, int n_frames, const float* d_plheader_phase,
                                   const float* d_phase_inc, const int32_t* d_coarse_corrected, const float* d_pilot_phase,
                                   float* d_xfecframes, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (int rc = check_frames(h, n_frames, d_payload && d_plheader_phase && d_phase_inc && d_coarse_corrected && d_xfecframes &&
                                           (h->impl->n_pilots() == 0 || d_pilot_phase))) return rc;
    return impl_rc(h, h->impl->process_device(d_payload, n_frames, d_plheader_phase, d_phase_inc, d_coarse_corrected, d_pilot_phase, d_xfecframes,
                                              (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plpayload_process(dvbs2_plpayload_t* h, const float* payload, int n_frames, const float* plheader_phase, const float* phase_inc,
                            const int32_t* coarse_corrected, const float* pilot_phase, float* xfecframes)
{
    API_TRY
    NEED_HANDLE(h);
    const int np = h->impl->n_pilots();
    if (int rc = check_frames(h, n_frames, payload && plheader_phase && phase_inc && coarse_corrected && xfecframes && (np == 0 || pilot_phase))) return rc;
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = h->impl->max_frames(), pl = h->impl->payload_len(), xl = h->impl->xfecframe_len(), nf = n_frames;
    if (s.ensure(h->IN, mf * pl * 8) || s.ensure(h->OUT, mf * xl * 8) || s.ensure(h->PAR, mf * (2 + (np ? np : 1)) * 4) || s.ensure(h->CC, mf * 4)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT); int32_t* d_cc = s.at<int32_t>(h->CC);
    float* d_hph = s.at<float>(h->PAR); float* d_inc = d_hph + mf; float* d_pp = d_hph + 2 * mf;
    HCHK(hipMemcpyAsync(d_in, payload, nf * pl * 8, hipMemcpyHostToDevice, s.stream));
    HCHK(hipMemcpyAsync(d_hph, plheader_phase, nf * 4, hipMemcpyHostToDevice, s.stream));
    HCHK(hipMemcpyAsync(d_inc, phase_inc, nf * 4, hipMemcpyHostToDevice, s.stream));
    HCHK(hipMemcpyAsync(d_cc, coarse_corrected, nf * 4, hipMemcpyHostToDevice, s.stream));
    if (np) HCHK(hipMemcpyAsync(d_pp, pilot_phase, nf * np * 4, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, n_frames, d_hph, d_inc, d_cc, d_pp, d_out, s.stream))) return rc;
    HCHK(hipMemcpyAsync(xfecframes, d_out, nf * xl * 8, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
