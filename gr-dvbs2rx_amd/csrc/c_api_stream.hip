// c_api_stream.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the stages that work on a running stream -- AGC, rotator, symbol
// timing recovery, pulse shaping, BBFRAME de-header and BB framing.
#include <algorithm>
#include <vector>
#include "c_api_common.h"
#include "fec_tables.h"
#include "agc_hip.h"
#include "rotator_hip.h"
#include "symsync_hip.h"
#include "pulse_hip.h"
#include "bbdeheader_hip.h"
#include "bbframer_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ AGC */
struct dvbs2_agc {
    AgcHip* impl = nullptr;
    HostStage stage; enum { BUF, GAIN, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kAgcTile == DVBS2_AGC_TILE, "the header names the kernel's tile");

// the checks the two work entries share; *done: nothing to do
static int agc_check_call(const dvbs2_agc_t* h, const void* in, int n_samples, int n_streams, const void* out, bool* done)
{
    *done = false;
    if (n_samples < 0) return fail(DVBS2_EINVAL, "n_samples is negative");
    if (n_streams < 0) return fail(DVBS2_EINVAL, "n_streams is negative");
    if (n_samples > h->impl->max_samples()) return fail(DVBS2_ESIZE, "n_samples exceeds max_samples");
    if (n_streams > h->impl->max_streams()) return fail(DVBS2_ESIZE, "n_streams exceeds max_streams");
    if (n_samples == 0 || n_streams == 0) { *done = true; return DVBS2_OK; }
    if (!in) return fail(DVBS2_EINVAL, "in is null");
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_agc_check(float rate, float reference, float gain, float max_gain)
{
    API_TRY
    const std::string bad = agc_check(rate, reference, gain, max_gain);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_agc_create(dvbs2_agc_t** h, float rate, float reference, float gain, float max_gain, int max_streams, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = AgcHip::check_args(rate, reference, gain, max_gain, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) AgcHip(rate, reference, gain, max_gain, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_agc_destroy(dvbs2_agc_t* h) { destroy_handle(h); }

int dvbs2_agc_reset(dvbs2_agc_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_agc_set_params(dvbs2_agc_t* h, float rate, float reference, float max_gain)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_params(rate, reference, max_gain));
    API_CATCH
}

int dvbs2_agc_set_swap_iq(dvbs2_agc_t* h, int enable)
{
    NEED_HANDLE(h);
    h->impl->set_swap_iq(enable != 0);
    return DVBS2_OK;
}

int dvbs2_agc_set_gain(dvbs2_agc_t* h, int stream_index, float gain)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_gain(stream_index, gain));
    API_CATCH
}

int dvbs2_agc_params(const dvbs2_agc_t* h, float* rate, float* reference, float* max_gain, int* swap_iq, int* tile)
{
    NEED_HANDLE(h);
    if (rate) *rate = h->impl->rate();
    if (reference) *reference = h->impl->reference();
    if (max_gain) *max_gain = h->impl->max_gain();
    if (swap_iq) *swap_iq = h->impl->swap_iq() ? 1 : 0;
    if (tile) *tile = kAgcTile;
    return DVBS2_OK;
}

int dvbs2_agc_state(dvbs2_agc_t* h, float* gains, int n_streams)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->state(gains, n_streams));
    API_CATCH
}

int dvbs2_agc_work_device(dvbs2_agc_t* h, const float* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out, int64_t out_stride,
                          float* d_gain, int64_t gain_stride, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = agc_check_call(h, d_in, n_samples, n_streams, d_out, &done)) return rc;
    if (done) return DVBS2_OK;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) return fail(DVBS2_EINVAL, "in and out must be 8-byte aligned");
    if ((uintptr_t)d_gain & 3) return fail(DVBS2_EINVAL, "gain must be 4-byte aligned");
    if (n_streams > 1 && in_stride < n_samples) return fail(DVBS2_EINVAL, "in_stride is below n_samples");
    if (n_streams > 1 && out_stride < n_samples) return fail(DVBS2_EINVAL, "out_stride is below n_samples");
    if (n_streams > 1 && d_gain && gain_stride < n_samples) return fail(DVBS2_EINVAL, "gain_stride is below n_samples");
    return impl_rc(h, h->impl->work_device(d_in, in_stride, n_samples, n_streams, d_out, out_stride, d_gain, gain_stride, (hipStream_t)stream));
    API_CATCH
}

// host entry, stream 0 of the handle: stage, run in place, copy back
int dvbs2_agc_work(dvbs2_agc_t* h, const float* in, int n_samples, float* out, float* gain)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = agc_check_call(h, in, n_samples, 1, out, &done)) return rc;
    if (done) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t bytes = (size_t)n_samples * 8;
    if (s.ensure(h->BUF, bytes) || (gain && s.ensure(h->GAIN, bytes / 2))) return DVBS2_EDEVICE;
    float* d_buf = s.at<float>(h->BUF); float* d_gain = gain ? s.at<float>(h->GAIN) : nullptr;
    HCHK(hipMemcpyAsync(d_buf, in, bytes, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->work_device(d_buf, n_samples, n_samples, 1, d_buf, n_samples, d_gain, n_samples, s.stream))) return rc;
    HCHK(hipMemcpyAsync(out, d_buf, bytes, hipMemcpyDeviceToHost, s.stream));
    if (gain) HCHK(hipMemcpyAsync(gain, d_gain, bytes / 2, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ rotator */
struct dvbs2_rotator {
    RotatorHip* impl = nullptr;
    HostStage stage; enum { BUF, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

extern "C" {

int dvbs2_rotator_create(dvbs2_rotator_t** h, double phase_inc, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    if (!(phase_inc == phase_inc) || phase_inc - phase_inc != 0.0) return fail(DVBS2_EINVAL, "phase_inc must be finite");
    return make_handle(h, device, [&] { return new (std::nothrow) RotatorHip(phase_inc, device); });
    API_CATCH
}

void dvbs2_rotator_destroy(dvbs2_rotator_t* h) { destroy_handle(h); }

int dvbs2_rotator_reset(dvbs2_rotator_t* h)
{
    NEED_HANDLE(h);
    h->impl->reset();
    return DVBS2_OK;
}

int dvbs2_rotator_set_phase_inc(dvbs2_rotator_t* h, double phase_inc)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_phase_inc(phase_inc));
    API_CATCH
}

int dvbs2_rotator_schedule(dvbs2_rotator_t* h, int64_t offset, double phase_inc)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->schedule(offset, phase_inc));
    API_CATCH
}

int dvbs2_rotator_seek(dvbs2_rotator_t* h, int64_t n_syms)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->seek(n_syms));
    API_CATCH
}

int dvbs2_rotator_position(const dvbs2_rotator_t* h, int64_t* n_syms, int* queued)
{
    NEED_HANDLE(h);
    if (n_syms) *n_syms = h->impl->position();
    if (queued) *queued = h->impl->queued();
    return DVBS2_OK;
}

int dvbs2_rotator_rotate_device(dvbs2_rotator_t* h, const float* d_in, int n_syms, float* d_out, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || (n_syms && (!d_in || !d_out))) return fail(DVBS2_EINVAL, "bad argument");
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) return fail(DVBS2_EINVAL, "symbol buffers must be 8-byte aligned");
    return impl_rc(h, h->impl->rotate_device(d_in, n_syms, d_out, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_rotator_measure(int device, int n_syms, int regions, double* rotate_ms, double* copy_ms)
{
    API_TRY
    if (!rotate_ms || !copy_ms) return fail(DVBS2_EINVAL, "bad argument");
    if (int rc = check_device(device)) return rc;
    std::string err;
    if (int rc = rotator_measure(device, n_syms, regions, rotate_ms, copy_ms, &err)) return fail(rc, err);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_rotate(dvbs2_rotator_t* h, const float* in, int n_syms, float* out)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || (n_syms && (!in || !out))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t bytes = (size_t)n_syms * 8;
    if (int rc = s.ensure(h->BUF, bytes)) return rc;
    float* d_buf = s.at<float>(h->BUF);
    HCHK(hipMemcpyAsync(d_buf, in, bytes, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->rotate_device(d_buf, n_syms, d_buf, s.stream))) return rc;
    HCHK(hipMemcpyAsync(out, d_buf, bytes, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"

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

/* ------------------------------------------------------------------ pulse shaping */
struct dvbs2_pulse {
    PulseShaperHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kPulseTile == DVBS2_PULSE_TILE, "the header names the kernel's tile");
static const char* const kPulseGeometryText = "sps must be an even integer in 2..64, rrc_delay in 1..64";

static int pulse_make(dvbs2_pulse_t** h, int sps, const float* taps, int ntaps, int max_streams, int max_symbols, int device)
{
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = PulseShaperHip::check_args(sps, taps, ntaps, max_streams, max_symbols);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) PulseShaperHip(sps, taps, ntaps, max_streams, max_symbols, device); });
}

// the checks the two shape entries share; *done: nothing to do
static int pulse_check(const dvbs2_pulse_t* h, const void* in, int n_syms, int n_streams, const void* out, bool* done)
{
    *done = false;
    if (n_syms < 0) return fail(DVBS2_EINVAL, "n_syms is negative");
    if (n_streams < 0) return fail(DVBS2_EINVAL, "n_streams is negative");
    if (n_syms > h->impl->max_symbols()) return fail(DVBS2_ESIZE, "n_syms exceeds max_symbols");
    if (n_streams > h->impl->max_streams()) return fail(DVBS2_ESIZE, "n_streams exceeds max_streams");
    if (n_syms == 0 || n_streams == 0) { *done = true; return DVBS2_OK; }
    if (!in) return fail(DVBS2_EINVAL, "in is null");
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_pulse_geometry(int sps, int rrc_delay, int* ntaps, int* history, int* delay)
{
    if (pulse_geometry(sps, rrc_delay, ntaps, history, delay)) return fail(DVBS2_EINVAL, kPulseGeometryText);
    return DVBS2_OK;
}

int dvbs2_pulse_taps(int sps, float rolloff, int rrc_delay, double tau, double gain, float* taps)
{
    if (!taps) return fail(DVBS2_EINVAL, "null taps");
    if (pulse_geometry(sps, rrc_delay, nullptr, nullptr, nullptr)) return fail(DVBS2_EINVAL, kPulseGeometryText);
    if (pulse_taps(sps, rolloff, rrc_delay, tau, gain, taps))
        return fail(DVBS2_EINVAL, "rolloff must lie in [0, 1], tau in [-0.5, 0.5], gain must be finite and not zero");
    return DVBS2_OK;
}

int dvbs2_pulse_scale_taps(float* taps, int ntaps, int sps, double fullscale)
{
    if (pulse_scale_taps(taps, ntaps, sps, fullscale))
        return fail(DVBS2_EINVAL, "taps must be ntaps >= 1 finite values that are not all zero, sps >= 1, fullscale finite");
    return DVBS2_OK;
}

int dvbs2_pulse_create(dvbs2_pulse_t** h, int sps, float rolloff, int rrc_delay, int max_streams, int max_symbols, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    int ntaps;
    if (pulse_geometry(sps, rrc_delay, &ntaps, nullptr, nullptr)) return fail(DVBS2_EINVAL, kPulseGeometryText);
    std::vector<float> taps(ntaps);
    if (pulse_taps(sps, rolloff, rrc_delay, 0.0, (double)sps, taps.data())) return fail(DVBS2_EINVAL, "rolloff must lie in [0, 1]");
    return pulse_make(h, sps, taps.data(), ntaps, max_streams, max_symbols, device);
    API_CATCH
}

int dvbs2_pulse_create_taps(dvbs2_pulse_t** h, int sps, const float* taps, int ntaps, int max_streams, int max_symbols, int device)
{
    API_TRY
    return pulse_make(h, sps, taps, ntaps, max_streams, max_symbols, device);
    API_CATCH
}

void dvbs2_pulse_destroy(dvbs2_pulse_t* h) { destroy_handle(h); }

int dvbs2_pulse_reset(dvbs2_pulse_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_pulse_params(const dvbs2_pulse_t* h, int* sps, int* ntaps, int* history, int* delay)
{
    NEED_HANDLE(h);
    if (sps) *sps = h->impl->sps();
    if (ntaps) *ntaps = h->impl->ntaps();
    if (history) *history = h->impl->history();
    if (delay) *delay = (h->impl->ntaps() - 1) / 2;
    return DVBS2_OK;
}

int dvbs2_pulse_shape_device(dvbs2_pulse_t* h, const float* d_in, int64_t in_stride, int n_syms, int n_streams, float* d_out, int64_t out_stride,
                             void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = pulse_check(h, d_in, n_syms, n_streams, d_out, &done)) return rc;
    if (done) return DVBS2_OK;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) return fail(DVBS2_EINVAL, "in and out must be 8-byte aligned");
    if (n_streams > 1 && in_stride < n_syms) return fail(DVBS2_EINVAL, "in_stride is below n_syms");
    if (n_streams > 1 && out_stride < (int64_t)n_syms * h->impl->sps()) return fail(DVBS2_EINVAL, "out_stride is below n_syms * sps");
    return impl_rc(h, h->impl->shape_device(d_in, in_stride, n_syms, n_streams, d_out, out_stride, (hipStream_t)stream));
    API_CATCH
}

// host entry, stream 0 of the handle: stage, run, copy back
int dvbs2_pulse_shape(dvbs2_pulse_t* h, const float* in, int n_syms, float* out)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = pulse_check(h, in, n_syms, 1, out, &done)) return rc;
    if (done) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t ib = (size_t)n_syms * 8, ob = ib * h->impl->sps();
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, ob)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, in, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->shape_device(d_in, n_syms, n_syms, 1, d_out, (int64_t)n_syms * h->impl->sps(), s.stream))) return rc;
    HCHK(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ BBFRAME de-header */
struct dvbs2_bbdeheader {
    BbDeheaderHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

extern "C" {

int dvbs2_bbdeheader_create_raw(dvbs2_bbdeheader_t** h, int kbch_bits, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, [&] { return new (std::nothrow) BbDeheaderHip(kbch_bits, max_frames, device); });
    API_CATCH
}

int dvbs2_bbdeheader_create(dvbs2_bbdeheader_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return dvbs2_bbdeheader_create_raw(h, (int)fi.bch_k, max_frames, device); // d_kbch_bytes, d_max_dfl (:58-61)
    API_CATCH
}

void dvbs2_bbdeheader_destroy(dvbs2_bbdeheader_t* h) { destroy_handle(h); }

int dvbs2_bbdeheader_params(const dvbs2_bbdeheader_t* h, int* kbch_bytes, int* max_dfl_bits, int* max_out_bytes_per_frame)
{
    NEED_HANDLE(h);
    if (kbch_bytes) *kbch_bytes = h->impl->kbch_bytes();
    if (max_dfl_bits) *max_dfl_bits = h->impl->max_dfl();
    if (max_out_bytes_per_frame) *max_out_bytes_per_frame = h->impl->max_out_bytes_per_frame();
    return DVBS2_OK;
}

int dvbs2_bbdeheader_process_device(dvbs2_bbdeheader_t* h, const uint8_t* d_bbframes, int n_frames, uint8_t* d_ts_out, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_bbframes && d_ts_out)) return rc;
    return impl_rc(h, h->impl->process_device(d_bbframes, n_frames, d_ts_out, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbdeheader_finish(dvbs2_bbdeheader_t* h, int64_t* produced, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    BbdhState st;
    if (int rc = impl_rc(h, h->impl->state(&st, (hipStream_t)stream))) return rc;
    if (produced) *produced = (int64_t)st.produced;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_counters(dvbs2_bbdeheader_t* h, dvbs2_bbdeheader_counters_t* out, void* stream)
{
    API_TRY
    if (!h || !out) return fail(DVBS2_EINVAL, "bad argument");
    BbdhState st;
    if (int rc = impl_rc(h, h->impl->state(&st, (hipStream_t)stream))) return rc;
    out->packets = st.packets; out->errors = st.errors; out->bbframes = st.bbframes; out->dropped = st.dropped; out->gaps = st.gaps;
    out->overruns = st.overruns; out->synched = st.synched; out->partial_ts_bytes = st.partial;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_reset(dvbs2_bbdeheader_t* h, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset((hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbdeheader_process(dvbs2_bbdeheader_t* h, const uint8_t* bbframes, int n_frames, uint8_t* ts_out, int64_t* produced)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, bbframes && ts_out)) return rc;
    if (produced) *produced = 0;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = h->impl->max_frames(), fb = h->impl->kbch_bytes(), ob = h->impl->max_out_bytes_per_frame();
    if (s.ensure(h->IN, mf * fb) || s.ensure(h->OUT, mf * ob)) return DVBS2_EDEVICE;
    uint8_t* d_in = s.at<uint8_t>(h->IN); uint8_t* d_out = s.at<uint8_t>(h->OUT);
    if (n_frames) HCHK(hipMemcpyAsync(d_in, bbframes, (size_t)n_frames * fb, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, n_frames, d_out, s.stream))) return rc;
    BbdhState st;
    if (int rc = impl_rc(h, h->impl->state(&st, s.stream))) return rc;
    if (st.produced > 0) {
        HCHK(hipMemcpyAsync(ts_out, d_out, (size_t)st.produced, hipMemcpyDeviceToHost, s.stream));
        if (int rc = s.sync()) return rc;
    }
    if (produced) *produced = (int64_t)st.produced;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"

/* ------------------------------------------------------------------ BB framing */
struct dvbs2_bbframer {
    BbFramerHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

extern "C" {

int dvbs2_bbframer_create_raw(dvbs2_bbframer_t** h, int kbch_bits, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = bbframer_check_create(kbch_bits, max_frames);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) BbFramerHip(kbch_bits, max_frames, device); });
    API_CATCH
}

int dvbs2_bbframer_create(dvbs2_bbframer_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return dvbs2_bbframer_create_raw(h, (int)fi.bch_k, max_frames, device);
    API_CATCH
}

void dvbs2_bbframer_destroy(dvbs2_bbframer_t* h) { destroy_handle(h); }

int dvbs2_bbframer_params(const dvbs2_bbframer_t* h, int* kbch_bytes, int* max_dfl_bytes, int* max_packets_per_call)
{
    NEED_HANDLE(h);
    if (kbch_bytes) *kbch_bytes = h->impl->kbch_bytes();
    if (max_dfl_bytes) *max_dfl_bytes = h->impl->max_dfl_bytes();
    if (max_packets_per_call) *max_packets_per_call = h->impl->max_packets_per_call();
    return DVBS2_OK;
}

int dvbs2_bbframer_set_matype(dvbs2_bbframer_t* h, int matype1, int matype2)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_matype(matype1, matype2));
    API_CATCH
}

int dvbs2_bbframer_need(const dvbs2_bbframer_t* h, int n_frames, int dfl_bytes, int* n_packets)
{
    API_TRY
    NEED_HANDLE(h);
    if (!n_packets) return fail(DVBS2_EINVAL, "n_packets is null");
    return impl_rc(h, h->impl->need(n_frames, dfl_bytes, n_packets));
    API_CATCH
}

int dvbs2_bbframer_process_device(dvbs2_bbframer_t* h, const uint8_t* d_ts, int n_frames, int dfl_bytes, uint8_t* d_bbframes, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->process_device(d_ts, n_frames, dfl_bytes, d_bbframes, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbframer_process(dvbs2_bbframer_t* h, const uint8_t* ts, int n_frames, int dfl_bytes, uint8_t* bbframes, int* n_packets_read)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_packets_read) *n_packets_read = 0;
    int n_pkts = 0;
    if (int rc = impl_rc(h, h->impl->need(n_frames, dfl_bytes, &n_pkts))) return rc;
    if (n_frames == 0) return DVBS2_OK;
    if (!ts) return fail(DVBS2_EINVAL, "ts is null");
    if (!bbframes) return fail(DVBS2_EINVAL, "bbframes is null");
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t ib = (size_t)n_pkts * kBbfTsLen, ob = (size_t)n_frames * h->impl->kbch_bytes();
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, ob)) return DVBS2_EDEVICE;
    uint8_t* d_in = s.at<uint8_t>(h->IN); uint8_t* d_out = s.at<uint8_t>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, ts, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, n_frames, dfl_bytes, d_out, s.stream))) return rc;
    HCHK(hipMemcpyAsync(bbframes, d_out, ob, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_packets_read) *n_packets_read = n_pkts;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbframer_counters(dvbs2_bbframer_t* h, dvbs2_bbframer_counters_t* out, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    BbfCounters c;
    if (int rc = impl_rc(h, h->impl->counters(&c, (hipStream_t)stream))) return rc;
    out->packets = c.packets; out->bbframes = c.bbframes; out->sync_errors = c.sync_errors;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbframer_reset(dvbs2_bbframer_t* h, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset((hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbheader_build(uint8_t out[10], int matype1, int matype2, int upl_bits, int dfl_bits, int sync, int syncd_bits)
{
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    if (bbheader_build(out, matype1, matype2, upl_bits, dfl_bits, sync, syncd_bits))
        return fail(DVBS2_EINVAL, "matype1, matype2 and sync must be in 0..255, upl_bits, dfl_bits and syncd_bits in 0..65535");
    return DVBS2_OK;
}

int dvbs2_crc8(const uint8_t* data, size_t n)
{
    if (!data && n) return fail(DVBS2_EINVAL, "data is null");
    return crc8(data, n);
}

} // extern "C"
