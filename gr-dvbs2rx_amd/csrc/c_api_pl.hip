// c_api_pl.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the physical-layer frame stages -- PLFRAME payload step, PLFRAME front
// end, PLFRAME search, coarse frequency estimate and, in the forward direction, the PL framer.
#include "c_api_common.h"
#include "plpayload_hip.h"
#include "plframe_hip.h"
#include "plsync_hip.h"
#include "plcoarse_hip.h"
#include "plframer_hip.h"

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

/* ------------------------------------------------------------------ PLFRAME search: timing metric, lock state machine, gather */
struct dvbs2_plsync {
    PlSyncHip* impl = nullptr;
    HostStage stage; enum { IN, FRAMES, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};
static_assert(sizeof(dvbs2_plsync_frame_t) == sizeof(PlSyncFrame) && offsetof(dvbs2_plsync_frame_t, metric) == offsetof(PlSyncFrame, metric) &&
              offsetof(dvbs2_plsync_frame_t, plsc) == offsetof(PlSyncFrame, plsc) && offsetof(dvbs2_plsync_frame_t, flags) == offsetof(PlSyncFrame, flags),
              "the public frame record is the kernel's");

extern "C" {

int dvbs2_plsync_taps(float* sof25, float* plsc32)
{
    if (!sof25 || !plsc32) return fail(DVBS2_EINVAL, "bad argument");
    plsync_taps(sof25, plsc32);
    return DVBS2_OK;
}

int dvbs2_plsync_thresholds(float* unlocked, float* locked)
{
    if (unlocked) *unlocked = kPlsyncThresholdUnlocked;
    if (locked) *locked = kPlsyncThresholdLocked;
    return DVBS2_OK;
}

int dvbs2_plsync_create(dvbs2_plsync_t** h, int plsc_or_minus1, int unlock_thresh, int max_symbols, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return fail(DVBS2_EINVAL, "plsc out of range (-1 = decode every header, 0..127)");
    if (unlock_thresh < 1 || unlock_thresh > 255) return fail(DVBS2_EINVAL, "unlock_thresh out of range (1..255)");
    if (max_symbols < kPlsyncMinSymbols) return fail(DVBS2_EINVAL, "max_symbols must be at least 33282 + 90");
    if (max_frames < 1 || max_frames > (1 << 20)) return fail(DVBS2_EINVAL, "max_frames out of range (1..1048576)");
    return make_handle(h, device, [&] { return new (std::nothrow) PlSyncHip(plsc_or_minus1, unlock_thresh, max_symbols, max_frames, device); });
    API_CATCH
}

void dvbs2_plsync_destroy(dvbs2_plsync_t* h) { destroy_handle(h); }

int dvbs2_plsync_reset(dvbs2_plsync_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_plsync_set_plsc_mode(dvbs2_plsync_t* h, int coherent, int soft)
{
    NEED_HANDLE(h);
    h->impl->set_plsc_mode(coherent, soft);
    return DVBS2_OK;
}

int dvbs2_plsync_set_expected_pls(dvbs2_plsync_t* h, const uint8_t* plsc_list, int n)
{
    API_TRY
    NEED_HANDLE(h);
    if (n < 0 || (n > 0 && !plsc_list)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->set_expected_pls(plsc_list, n));
    API_CATCH
}

int dvbs2_plsync_metric_device(dvbs2_plsync_t* h, const float* d_syms, int n_syms, float* d_metric, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || (n_syms && (!d_syms || !d_metric))) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->metric_device(d_syms, n_syms, d_metric, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plsync_search_device(dvbs2_plsync_t* h, const float* d_syms, int n_syms, dvbs2_plsync_frame_t* d_frames, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || !d_frames || (n_syms && !d_syms)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms > h->impl->max_symbols()) return fail(DVBS2_ESIZE, "n_syms exceeds max_symbols");
    return impl_rc(h, h->impl->search_device(d_syms, n_syms, reinterpret_cast<PlSyncFrame*>(d_frames), (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plsync_finish(dvbs2_plsync_t* h, int* n_frames, int* consumed, int* state)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->finish(n_frames, consumed, state));
    API_CATCH
}

int dvbs2_plsync_search(dvbs2_plsync_t* h, const float* syms, int n_syms, dvbs2_plsync_frame_t* frames, int* n_frames, int* consumed, int* state)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || !frames || (n_syms && !syms)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms > h->impl->max_symbols()) return fail(DVBS2_ESIZE, "n_syms exceeds max_symbols");
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    if (s.ensure(h->IN, (size_t)h->impl->max_symbols() * 8) || s.ensure(h->FRAMES, (size_t)h->impl->max_frames() * sizeof(PlSyncFrame))) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); PlSyncFrame* d_frames = s.at<PlSyncFrame>(h->FRAMES);
    if (n_syms) HCHK(hipMemcpyAsync(d_in, syms, (size_t)n_syms * 8, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->search_device(d_in, n_syms, d_frames, s.stream))) return rc;
    int nf = 0;
    if (int rc = impl_rc(h, h->impl->finish(&nf, consumed, state))) return rc;
    if (nf) HCHK(hipMemcpy(frames, d_frames, (size_t)nf * sizeof(PlSyncFrame), hipMemcpyDeviceToHost));
    if (n_frames) *n_frames = nf;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plsync_gather_device(dvbs2_plsync_t* h, const float* d_syms, const dvbs2_plsync_frame_t* d_frames, int n_frames, int wanted_plsc,
                               float* d_plframes, int32_t* d_count, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (wanted_plsc < 0 || wanted_plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    if (int rc = check_frames(h, n_frames, d_syms && d_frames && d_plframes, !d_count)) return rc;
    return impl_rc(h, h->impl->gather_device(d_syms, reinterpret_cast<const PlSyncFrame*>(d_frames), n_frames, wanted_plsc, d_plframes, d_count, (hipStream_t)stream));
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ coarse frequency offset estimate */
struct dvbs2_plcoarse {
    PlCoarseHip* impl = nullptr;
    HostStage stage; enum { HDR, PLSC, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

static PlCoarseOut plcoarse_out(float* foffset, int32_t* corrected, int32_t* new_est)
{
    PlCoarseOut o;
    o.foffset = foffset; o.corrected = corrected; o.new_est = new_est;
    return o;
}

extern "C" {

int dvbs2_plcoarse_weights(int full, float* w)
{
    if (!w) return fail(DVBS2_EINVAL, "bad argument");
    return plcoarse_weights(full, w);
}

int dvbs2_plcoarse_create(dvbs2_plcoarse_t** h, int period, int plsc_or_minus1, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (period < 1) return fail(DVBS2_EINVAL, "period must be at least 1");
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return fail(DVBS2_EINVAL, "plsc out of range (-1 = not known, 0..127)");
    if (max_frames < 1 || max_frames > (1 << 20)) return fail(DVBS2_EINVAL, "max_frames out of range (1..1048576)");
    return make_handle(h, device, [&] { return new (std::nothrow) PlCoarseHip(period, plsc_or_minus1, max_frames, device); });
    API_CATCH
}

void dvbs2_plcoarse_destroy(dvbs2_plcoarse_t* h) { destroy_handle(h); }

int dvbs2_plcoarse_reset(dvbs2_plcoarse_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_plcoarse_estimate_device(dvbs2_plcoarse_t* h, const float* d_plframes, int64_t stride_syms, const uint8_t* d_plsc, int n_frames,
                                   float* d_coarse_foffset, int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_plframes)) return rc;
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!d_plsc && h->impl->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array");
    return impl_rc(h, h->impl->frames_device(d_plframes, stride_syms, d_plsc, n_frames, plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est),
                                             (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plcoarse_estimate_records_device(dvbs2_plcoarse_t* h, const float* d_syms, int n_syms, int64_t base_index,
                                           const dvbs2_plsync_frame_t* d_frames, int n_frames, float* d_coarse_foffset,
                                           int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_frames)) return rc;
    if (n_syms < 0 || (n_frames && !d_syms)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->records_device(d_syms, n_syms, reinterpret_cast<const PlSyncFrame*>(d_frames), n_frames, base_index,
                                              plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est), (hipStream_t)stream));
    API_CATCH
}

// host entry: stage the 90 header symbols of every frame, run, copy back what the caller asked for
int dvbs2_plcoarse_estimate(dvbs2_plcoarse_t* h, const float* plframes, int64_t stride_syms, const uint8_t* plsc, int n_frames,
                            float* coarse_foffset, int32_t* coarse_corrected, int32_t* new_est)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, plframes)) return rc;
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!plsc && h->impl->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array");
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = h->impl->max_frames(), nf = n_frames;
    if (s.ensure(h->HDR, mf * 90 * 8) || s.ensure(h->PLSC, mf) || s.ensure(h->OUT, mf * 3 * 4)) return DVBS2_EDEVICE;
    float* d_hdr = s.at<float>(h->HDR); uint8_t* d_plsc = s.at<uint8_t>(h->PLSC);
    float* d_fo = s.at<float>(h->OUT); int32_t* d_cc = s.at<int32_t>(h->OUT) + mf; int32_t* d_ne = s.at<int32_t>(h->OUT) + 2 * mf;
    HCHK(hipMemcpy2DAsync(d_hdr, 90 * 8, plframes, (size_t)stride_syms * 8, 90 * 8, nf, hipMemcpyHostToDevice, s.stream));
    if (plsc) HCHK(hipMemcpyAsync(d_plsc, plsc, nf, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->frames_device(d_hdr, 90, plsc ? d_plsc : nullptr, n_frames, plcoarse_out(d_fo, d_cc, d_ne), s.stream))) return rc;
    if (coarse_foffset) HCHK(hipMemcpyAsync(coarse_foffset, d_fo, nf * 4, hipMemcpyDeviceToHost, s.stream));
    if (coarse_corrected) HCHK(hipMemcpyAsync(coarse_corrected, d_cc, nf * 4, hipMemcpyDeviceToHost, s.stream));
    if (new_est) HCHK(hipMemcpyAsync(new_est, d_ne, nf * 4, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ PL framer: XFECFRAMEs -> PLFRAMEs (PLHEADER, pilots, PL scrambling) */
struct dvbs2_plframer {
    PlFramerHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

// the checks the two framing entries share; buffers are checked for n_frames > 0 only, the input only where a data frame reads it
static int plframer_check(const dvbs2_plframer* h, const void* xfecframes, int n_frames, int closing_plsc, const void* plframes)
{
    NEED_HANDLE(h);
    if (n_frames < 0) return fail(DVBS2_EINVAL, "n_frames is negative");
    if (closing_plsc < -1 || closing_plsc > 127) return fail(DVBS2_EINVAL, "closing_plsc out of range (-1 = none, 0..127)");
    if (closing_plsc >= 0) if (const char* why = plframer_refusal(closing_plsc)) return fail(DVBS2_EINVAL, std::string("closing_plsc ") + why);
    if (n_frames > h->impl->n_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds the sequence");
    if (n_frames && !plframes) return fail(DVBS2_EINVAL, "plframes is null");
    if (n_frames && !xfecframes && h->impl->in_end(n_frames) > 0) return fail(DVBS2_EINVAL, "xfecframes is null and the framed prefix holds a data frame");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_plframer_layout(const uint8_t* plsc, int n_frames, int64_t* in_offset, int64_t* out_offset, int64_t* in_syms, int64_t* out_syms)
{
    API_TRY
    if (n_frames < 0 || (n_frames && !plsc)) return fail(DVBS2_EINVAL, "bad argument");
    std::vector<PlFramerRec> rec(n_frames);
    std::string why;
    if (!plframer_layout(plsc, n_frames, rec.data(), in_syms, out_syms, &why)) return fail(DVBS2_EINVAL, why);
    for (int f = 0; f < n_frames; f++) {
        if (in_offset) in_offset[f] = rec[f].in_offset;
        if (out_offset) out_offset[f] = rec[f].out_offset;
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plframer_create(dvbs2_plframer_t** h, int gold_code, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, [&] { return new (std::nothrow) PlFramerHip(gold_code, max_frames, device); });
    API_CATCH
}

void dvbs2_plframer_destroy(dvbs2_plframer_t* h) { destroy_handle(h); }

int dvbs2_plframer_set_sequence(dvbs2_plframer_t* h, const uint8_t* plsc, int n_frames)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_frames < 0 || (n_frames && !plsc)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->set_sequence(plsc, n_frames));
    API_CATCH
}

int dvbs2_plframer_params(const dvbs2_plframer_t* h, int* n_frames, int64_t* in_syms, int64_t* out_syms)
{
    NEED_HANDLE(h);
    if (n_frames) *n_frames = h->impl->n_frames();
    if (in_syms) *in_syms = h->impl->in_syms();
    if (out_syms) *out_syms = h->impl->out_syms();
    return DVBS2_OK;
}

int dvbs2_plframer_frame_device(dvbs2_plframer_t* h, const float* d_xfecframes, int n_frames, int closing_plsc, float* d_plframes, void* stream)
{
    API_TRY
    if (int rc = plframer_check(h, d_xfecframes, n_frames, closing_plsc, d_plframes)) return rc;
    return impl_rc(h, h->impl->frame_device(d_xfecframes, n_frames, closing_plsc, d_plframes, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plframer_frame(dvbs2_plframer_t* h, const float* xfecframes, int n_frames, int closing_plsc, float* plframes)
{
    API_TRY
    if (int rc = plframer_check(h, xfecframes, n_frames, closing_plsc, plframes)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    // sized for the sequence as it is set: the buffers grow when a longer one follows
    const size_t in_bytes = (size_t)h->impl->in_end(n_frames) * 8, out_bytes = ((size_t)h->impl->out_end(n_frames) + (closing_plsc >= 0 ? 90 : 0)) * 8;
    if (s.ensure(h->IN, (size_t)h->impl->in_syms() * 8 + 16) || s.ensure(h->OUT, ((size_t)h->impl->out_syms() + 90) * 8)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    if (in_bytes) HCHK(hipMemcpyAsync(d_in, xfecframes, in_bytes, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->frame_device(d_in, n_frames, closing_plsc, d_out, s.stream))) return rc;
    HCHK(hipMemcpyAsync(plframes, d_out, out_bytes, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
