// c_api_resamp.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): arbitrary-rate resampling of a running stream.
#include <algorithm>
#include <vector>
#include "c_api_common.h"
#include "resamp_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ arbitrary-rate resampling */
struct dvbs2_resamp {
    ResamplerHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kResampTile == DVBS2_RESAMP_TILE, "the header names the kernel's tile");
static const char* const kResampStepText = "step must lie in [2^26, 2^33]";

extern "C" {

int dvbs2_resamp_step(double rate, uint64_t* step)
{
    if (!step) return fail(DVBS2_EINVAL, "null step");
    if (resamp_step(rate, step)) return fail(DVBS2_EINVAL, "rate must lie in [0.5, 64]");
    return DVBS2_OK;
}

int dvbs2_resamp_geometry(int nfilts, int ntaps, int* terms, int* history, int* delay_num)
{
    if (resamp_geometry(nfilts, ntaps, terms, history, delay_num))
        return fail(DVBS2_EINVAL, "nfilts must be a power of two in 2..256, ntaps in 1..8192 with ceil(ntaps / nfilts) <= 128");
    return DVBS2_OK;
}

int64_t dvbs2_resamp_max_out(uint64_t step, int n_in)
{
    const int64_t n = resamp_max_out(step, n_in);
    if (n < 0) return fail(DVBS2_EINVAL, "step must lie in [2^26, 2^33], n_in in 0..2^24");
    return n;
}

int dvbs2_resamp_check(int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples)
{
    const std::string bad = ResamplerHip::check_args(nfilts, taps, ntaps, rate, max_streams, max_samples);
    return bad.empty() ? DVBS2_OK : fail(DVBS2_EINVAL, bad);
}

int dvbs2_resamp_create(dvbs2_resamp_t** h, int nfilts, const float* taps, int ntaps, double rate, int max_streams, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (int rc = dvbs2_resamp_check(nfilts, taps, ntaps, rate, max_streams, max_samples)) return rc;
    return make_handle(h, device, [&] { return new (std::nothrow) ResamplerHip(nfilts, taps, ntaps, rate, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_resamp_destroy(dvbs2_resamp_t* h) { destroy_handle(h); }

int dvbs2_resamp_reset(dvbs2_resamp_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_resamp_reset_phase(dvbs2_resamp_t* h, const uint32_t* frac)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset_phase(frac));
    API_CATCH
}

int dvbs2_resamp_set_step(dvbs2_resamp_t* h, uint64_t step)
{
    NEED_HANDLE(h);
    if (h->impl->set_step(step)) return fail(DVBS2_EINVAL, kResampStepText);
    return DVBS2_OK;
}

int dvbs2_resamp_set_rate(dvbs2_resamp_t* h, double rate)
{
    NEED_HANDLE(h);
    uint64_t step;
    if (int rc = dvbs2_resamp_step(rate, &step)) return rc;
    return dvbs2_resamp_set_step(h, step);
}

int dvbs2_resamp_params(const dvbs2_resamp_t* h, int* nfilts, int* ntaps, int* terms, int* history, int* delay_num, uint64_t* step)
{
    NEED_HANDLE(h);
    if (nfilts) *nfilts = h->impl->nfilts();
    if (ntaps) *ntaps = h->impl->ntaps();
    if (terms) *terms = h->impl->terms();
    if (history) *history = h->impl->history();
    if (delay_num) *delay_num = (h->impl->ntaps() - 1) / 2;
    if (step) *step = h->impl->step();
    return DVBS2_OK;
}

int dvbs2_resamp_produce(const dvbs2_resamp_t* h, int n_in, int n_streams, int64_t* n_out)
{
    NEED_HANDLE(h);
    if (int rc = check_stream_counts(h, n_in, "n_in", "max_samples", n_streams)) return rc;
    if (n_streams && !n_out) return fail(DVBS2_EINVAL, "n_out is null");
    h->impl->produce(n_in, n_streams, n_out);
    return DVBS2_OK;
}

int dvbs2_resamp_state(dvbs2_resamp_t* h, uint64_t* acc)
{
    API_TRY
    NEED_HANDLE(h);
    if (!acc) return fail(DVBS2_EINVAL, "acc is null");
    return impl_rc(h, h->impl->state(acc));
    API_CATCH
}

int dvbs2_resamp_process_device(dvbs2_resamp_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out,
                                int64_t out_stride, int64_t* n_out_host, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = check_stream_call(h, d_in, n_in, "n_in", "max_samples", n_streams, d_out, &done)) return rc;
    if (done) { // (no output, positions unchanged)
        for (int s = 0; n_out_host && s < n_streams; s++) n_out_host[s] = 0;
        return DVBS2_OK;
    }
    if (int rc = check_aligned8(d_in, d_out)) return rc;
    if (n_streams > 1 && in_stride < n_in) return fail(DVBS2_EINVAL, "in_stride is below n_in");
    if (out_stride < h->impl->produce(n_in, n_streams, nullptr)) return fail(DVBS2_EINVAL, "out_stride is below the call's largest n_out");
    std::vector<int64_t> n_out((size_t)n_streams); // (before the launches: the mirror advances with them)
    h->impl->produce(n_in, n_streams, n_out.data());
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, (hipStream_t)stream))) return rc;
    if (n_out_host) std::copy(n_out.begin(), n_out.end(), n_out_host);
    return DVBS2_OK;
    API_CATCH
}

// host entry, stream 0 of the handle: stage, run, copy back
int dvbs2_resamp_process(dvbs2_resamp_t* h, const float* in, int n_in, float* out, int64_t out_cap, int64_t* n_out)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (n_out) *n_out = 0;
    if (out_cap < 0) return fail(DVBS2_EINVAL, "out_cap is negative");
    if (int rc = check_stream_call(h, in, n_in, "n_in", "max_samples", 1, out, &done)) return rc;
    if (done) return DVBS2_OK;
    int64_t n;
    h->impl->produce(n_in, 1, &n);
    if (out_cap < n) return fail(DVBS2_EINVAL, "out_cap is below n_out");
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t ib = (size_t)n_in * 8, ob = (size_t)n * 8;
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, std::max(ob, (size_t)8))) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, in, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, n_in, n_in, 1, d_out, n, s.stream))) return rc;
    if (n) HCHK(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_out) *n_out = n;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
