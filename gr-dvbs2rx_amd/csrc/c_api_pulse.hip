// c_api_pulse.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): pulse shaping.
#include <vector>
#include "c_api_common.h"
#include "pulse_hip.h"

using namespace dvbs2;

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
    if (int rc = check_stream_call(h, d_in, n_syms, "n_syms", "max_symbols", n_streams, d_out, &done)) return rc;
    if (done) return DVBS2_OK;
    if (int rc = check_aligned8(d_in, d_out)) return rc;
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
    if (int rc = check_stream_call(h, in, n_syms, "n_syms", "max_symbols", 1, out, &done)) return rc;
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
