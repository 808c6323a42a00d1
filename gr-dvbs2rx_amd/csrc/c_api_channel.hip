// c_api_channel.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the channel between the transmit and the receive stages -- the
// additive white Gaussian noise stage.
#include <cstdint>
#include "c_api_common.h"
#include "awgn_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ AWGN */
struct dvbs2_awgn {
    AwgnHip* impl = nullptr;
    HostStage stage; enum { BUF, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kAwgnTile == DVBS2_AWGN_TILE, "the header names the kernel's tile");

// the checks the two add entries share: first_index stands between the counts and *done (nothing to do); `in` may be null
static int awgn_check_call(const dvbs2_awgn_t* h, int n_samples, int n_streams, int64_t first_index, const void* out, bool* done)
{
    *done = false;
    if (int rc = check_stream_counts(h, n_samples, "n_samples", "max_samples", n_streams)) return rc;
    if (first_index < 0) return fail(DVBS2_EINVAL, "first_index is negative");
    if (first_index > INT64_MAX - n_samples) return fail(DVBS2_EINVAL, "first_index + n_samples passes 2^63 - 1");
    if (n_samples == 0 || n_streams == 0) { *done = true; return DVBS2_OK; }
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_awgn_sigma(double esn0_db, double es, int sps, float* sigma)
{
    API_TRY
    const std::string bad = awgn_sigma(esn0_db, es, sps, sigma);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_awgn_words(uint64_t seed, uint64_t stream_id, int64_t index, uint32_t* wa_wb)
{
    if (index < 0) return fail(DVBS2_EINVAL, "index is negative");
    if (!wa_wb) return fail(DVBS2_EINVAL, "wa_wb is null");
    awgn_words(seed, stream_id, index, wa_wb);
    return DVBS2_OK;
}

int dvbs2_awgn_sample(uint64_t seed, uint64_t stream_id, int64_t index, float* re_im)
{
    if (index < 0) return fail(DVBS2_EINVAL, "index is negative");
    if (!re_im) return fail(DVBS2_EINVAL, "re_im is null");
    awgn_sample(seed, stream_id, index, re_im);
    return DVBS2_OK;
}

int dvbs2_awgn_check(float sigma, int max_streams, int max_samples)
{
    API_TRY
    const std::string bad = awgn_check(sigma, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_awgn_create(dvbs2_awgn_t** h, uint64_t seed, float sigma, int max_streams, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = awgn_check(sigma, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) AwgnHip(seed, sigma, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_awgn_destroy(dvbs2_awgn_t* h) { destroy_handle(h); }

int dvbs2_awgn_set_sigma(dvbs2_awgn_t* h, float sigma)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_sigma(sigma));
    API_CATCH
}

int dvbs2_awgn_set_seed(dvbs2_awgn_t* h, uint64_t seed)
{
    NEED_HANDLE(h);
    h->impl->set_seed(seed);
    return DVBS2_OK;
}

int dvbs2_awgn_params(const dvbs2_awgn_t* h, uint64_t* seed, float* sigma, int* max_streams, int* max_samples)
{
    NEED_HANDLE(h);
    if (seed) *seed = h->impl->seed();
    if (sigma) *sigma = h->impl->sigma();
    if (max_streams) *max_streams = h->impl->max_streams();
    if (max_samples) *max_samples = h->impl->max_samples();
    return DVBS2_OK;
}

int dvbs2_awgn_add_device(dvbs2_awgn_t* h, const float* d_in, int64_t in_stride, int n_samples, int n_streams, uint64_t first_stream,
                          int64_t first_index, const float* d_sigma, float* d_out, int64_t out_stride, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = awgn_check_call(h, n_samples, n_streams, first_index, d_out, &done)) return rc;
    if (done) return DVBS2_OK;
    if (int rc = check_aligned8(d_in, d_out)) return rc;
    if ((uintptr_t)d_sigma & 3) return fail(DVBS2_EINVAL, "sigma must be 4-byte aligned");
    if (n_streams > 1 && d_in && in_stride < n_samples) return fail(DVBS2_EINVAL, "in_stride is below n_samples");
    if (n_streams > 1 && out_stride < n_samples) return fail(DVBS2_EINVAL, "out_stride is below n_samples");
    return impl_rc(h, h->impl->add_device(d_in, in_stride, n_samples, n_streams, first_stream, first_index, d_sigma, d_out, out_stride,
                                          (hipStream_t)stream));
    API_CATCH
}

// host entry, one row: stage (or not, for the noise alone), run in place, copy back
int dvbs2_awgn_add(dvbs2_awgn_t* h, const float* in, int n_samples, uint64_t stream_id, int64_t first_index, float* out)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = awgn_check_call(h, n_samples, 1, first_index, out, &done)) return rc;
    if (done) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t bytes = (size_t)n_samples * 8;
    if (s.ensure(h->BUF, bytes)) return DVBS2_EDEVICE;
    float* d_buf = s.at<float>(h->BUF);
    if (in) HCHK(hipMemcpyAsync(d_buf, in, bytes, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->add_device(in ? d_buf : nullptr, n_samples, n_samples, 1, stream_id, first_index, nullptr, d_buf, n_samples, s.stream)))
        return rc;
    HCHK(hipMemcpyAsync(out, d_buf, bytes, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
