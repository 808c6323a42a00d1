// c_api_agc.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the AGC, the first stage of the receive path.
#include "c_api_common.h"
#include "agc_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ AGC */
struct dvbs2_agc {
    AgcHip* impl = nullptr;
    HostStage stage; enum { BUF, GAIN, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kAgcTile == DVBS2_AGC_TILE, "the header names the kernel's tile");

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
    if (int rc = check_stream_call(h, d_in, n_samples, "n_samples", "max_samples", n_streams, d_out, &done)) return rc;
    if (done) return DVBS2_OK;
    if (int rc = check_aligned8(d_in, d_out)) return rc;
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
    if (int rc = check_stream_call(h, in, n_samples, "n_samples", "max_samples", 1, out, &done)) return rc;
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
