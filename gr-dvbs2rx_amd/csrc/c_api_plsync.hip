// c_api_plsync.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the PLFRAME search.
#include "c_api_common.h"
#include "plsync_hip.h"

using namespace dvbs2;

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
