// c_api_symsync.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): symbol timing recovery.
#include <algorithm>
#include "c_api_common.h"
#include "symsync_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ symbol timing recovery */
struct dvbs2_symsync {
    SymSyncHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, IDX, MU, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static int symsync_make(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp_method,
                        const float* bank, int max_streams, int max_samples, int device)
{
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = SymSyncHip::check_args(sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] {
        return new (std::nothrow) SymSyncHip(sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, bank, max_streams, max_samples, device);
    });
}

extern "C" {

int dvbs2_symsync_loop_constants(int sps, float loop_bw, float damping, float rolloff, float* Kp, float* K1, float* K2)
{
    if (sps < 2 || (sps & 1)) return fail(DVBS2_EINVAL, "sps has to be an even integer >= 2");
    symsync_loop_constants(sps, loop_bw, damping, rolloff, Kp, K1, K2);
    return DVBS2_OK;
}

int dvbs2_symsync_geometry(int sps, int rrc_delay, int n_subfilt, int interp_method, int* subfilt_len, int* subfilt_delay, int* history)
{
    if (symsync_geometry(sps, rrc_delay, n_subfilt, interp_method, subfilt_len, subfilt_delay, history)) return fail(DVBS2_EINVAL, "bad argument");
    return DVBS2_OK;
}

int dvbs2_symsync_taps(int sps, float rolloff, int rrc_delay, int n_subfilt, float* bank)
{
    API_TRY
    if (symsync_taps(sps, rolloff, rrc_delay, n_subfilt, bank)) return fail(DVBS2_EINVAL, "bad argument");
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_symsync_create(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt, int interp_method,
                         int max_streams, int max_samples, int device)
{
    API_TRY
    return symsync_make(h, sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, nullptr, max_streams, max_samples, device);
    API_CATCH
}

int dvbs2_symsync_create_taps(dvbs2_symsync_t** h, int sps, float loop_bw, float damping, float rolloff, int rrc_delay, int n_subfilt,
                              int interp_method, const float* bank, int max_streams, int max_samples, int device)
{
    API_TRY
    if (h) *h = nullptr;
    if (!bank) return fail(DVBS2_EINVAL, "null bank");
    return symsync_make(h, sps, loop_bw, damping, rolloff, rrc_delay, n_subfilt, interp_method, bank, max_streams, max_samples, device);
    API_CATCH
}

void dvbs2_symsync_destroy(dvbs2_symsync_t* h) { destroy_handle(h); }

int dvbs2_symsync_reset(dvbs2_symsync_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_symsync_params(const dvbs2_symsync_t* h, int* subfilt_len, int* subfilt_delay, int* history, float* Kp, float* K1, float* K2)
{
    NEED_HANDLE(h);
    const SymSyncGeom& g = h->impl->geom();
    if (subfilt_len) *subfilt_len = g.subfilt_len;
    if (subfilt_delay) *subfilt_delay = g.subfilt_delay;
    if (history) *history = g.history;
    if (Kp) *Kp = h->impl->Kp();
    if (K1) *K1 = g.K1;
    if (K2) *K2 = g.K2;
    return DVBS2_OK;
}

int dvbs2_symsync_work_device(dvbs2_symsync_t* h, const float* d_in, int64_t in_stride, const int* n_in, int n_streams, float* d_out,
                              int64_t out_stride, int max_out, int64_t* d_strobe_idx, double* d_mu, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_streams < 1 || !n_in || !d_in || max_out < 0 || (max_out && !d_out)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_streams > h->impl->max_streams()) return fail(DVBS2_ESIZE, "n_streams exceeds max_streams");
    if (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_strobe_idx | (uintptr_t)d_mu) & 7) return fail(DVBS2_EINVAL, "buffers must be 8-byte aligned");
    int most = 0;
    for (int s = 0; s < n_streams; s++) {
        if (n_in[s] < 0) return fail(DVBS2_EINVAL, "negative sample count");
        if (n_in[s] > h->impl->max_samples()) return fail(DVBS2_ESIZE, "n_in exceeds max_samples");
        most = std::max(most, n_in[s]);
    }
    if (n_streams > 1 && (in_stride < most || out_stride < max_out)) return fail(DVBS2_EINVAL, "a stride below the length of a stream");
    return impl_rc(h, h->impl->work_device(reinterpret_cast<const float2*>(d_in), in_stride, n_in, n_streams, reinterpret_cast<float2*>(d_out), out_stride, max_out,
                                           d_strobe_idx, d_mu, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_symsync_finish(dvbs2_symsync_t* h, int* n_out, int* consumed, int* status)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->finish(n_out, consumed, status) < 0);
    API_CATCH
}

int dvbs2_symsync_state(dvbs2_symsync_t* h, int stream_index, dvbs2_symsync_state_t* out)
{
    API_TRY
    if (!h || !out) return fail(DVBS2_EINVAL, "bad argument");
    if (stream_index < 0 || stream_index >= h->impl->max_streams()) return fail(DVBS2_EINVAL, "stream index out of range");
    SymSyncState s;
    if (int rc = impl_rc(h, h->impl->state(stream_index, &s))) return rc;
    out->vi = s.vi; out->cnt = s.cnt; out->mu = s.mu; out->n_read = s.n_read; out->last_xi_re = s.last_xi.x; out->last_xi_im = s.last_xi.y;
    out->jump = s.jump; out->init = s.init; out->status = s.status; out->reserved = 0;
    return DVBS2_OK;
    API_CATCH
}

// host entry, stream 0 of the handle: stage, run, copy back what the caller asked for
int dvbs2_symsync_work(dvbs2_symsync_t* h, const float* in, int n_in, float* out, int max_out, int64_t* strobe_idx, double* mu, int* n_out,
                       int* consumed, int* status)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_in < 0 || max_out < 0 || (n_in && !in) || (max_out && !out)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_in > h->impl->max_samples()) return fail(DVBS2_ESIZE, "n_in exceeds max_samples");
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t ni = std::max(n_in, 1), no = std::max(max_out, 1);
    if (s.ensure(h->IN, ni * 8) || s.ensure(h->OUT, no * 8) || s.ensure(h->IDX, no * 8) || s.ensure(h->MU, no * 8)) return DVBS2_EDEVICE;
    float2* d_in = s.at<float2>(h->IN); float2* d_out = s.at<float2>(h->OUT); int64_t* d_idx = s.at<int64_t>(h->IDX); double* d_mu = s.at<double>(h->MU);
    if (n_in) HCHK(hipMemcpyAsync(d_in, in, (size_t)n_in * 8, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->work_device(d_in, n_in, &n_in, 1, d_out, max_out, max_out, d_idx, d_mu, s.stream))) return rc;
    int k = 0, c = 0, st = 0;
    if (int rc = impl_rc(h, h->impl->finish(&k, &c, &st) < 0)) return rc;
    if (k) {
        HCHK(hipMemcpy(out, d_out, (size_t)k * 8, hipMemcpyDeviceToHost));
        if (strobe_idx) HCHK(hipMemcpy(strobe_idx, d_idx, (size_t)k * 8, hipMemcpyDeviceToHost));
        if (mu) HCHK(hipMemcpy(mu, d_mu, (size_t)k * 8, hipMemcpyDeviceToHost));
    }
    if (n_out) *n_out = k;
    if (consumed) *consumed = c;
    if (status) *status = st;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
