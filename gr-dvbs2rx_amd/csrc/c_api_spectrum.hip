// c_api_spectrum.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): power spectra of a batch of sample streams and the carrier finder
// over one row.
#include <algorithm>
#include <cstring>
#include "c_api_common.h"
#include "spectrum_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ spectrum estimate */
struct dvbs2_spectrum {
    SpectrumHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kSpectrumChunk == DVBS2_SPECTRUM_CHUNK, "the header names the kernel's chunk");
static_assert(kSpectrumRect == DVBS2_SPECTRUM_RECT && kSpectrumHann == DVBS2_SPECTRUM_HANN && kSpectrumHamming == DVBS2_SPECTRUM_HAMMING &&
              kSpectrumBlackmanHarris == DVBS2_SPECTRUM_BLACKMAN_HARRIS, "the header names the windows");
static_assert(sizeof(dvbs2_spectrum_carrier_params_t) == sizeof(SpectrumCarrierParams) && sizeof(dvbs2_spectrum_carrier_t) == sizeof(SpectrumCarrier),
              "the header's records are the finder's");

// the checks the work entries share, alignment apart; *done: no launch (no row, or no stream)
static int spectrum_check_call(const dvbs2_spectrum_t* h, const void* in, int64_t in_stride, int n_in, int n_streams, const void* out,
                               int64_t out_stride, int* n_rows, bool* done)
{
    const SpectrumHip& s = *h->impl;
    *done = false;
    if (int rc = check_stream_counts(h, n_in, "n_in", "max_samples", n_streams)) return rc;
    spectrum_geometry(s.nfft(), s.hop(), s.avg(), n_in, nullptr, n_rows, nullptr);
    if (*n_rows == 0 || n_streams == 0) { *done = true; return DVBS2_OK; }
    if (int rc = check_in_out(in, out)) return rc;
    if (n_streams > 1 && in_stride < n_in) return fail(DVBS2_EINVAL, "in_stride is below n_in");
    if (out_stride < (int64_t)*n_rows * s.nfft()) return fail(DVBS2_EINVAL, "out_stride is below n_rows nfft");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_spectrum_geometry(int nfft, int hop, int avg, int n_in, int* n_seg, int* n_rows, int* used_samples)
{
    if (spectrum_geometry(nfft, hop, avg, n_in, n_seg, n_rows, used_samples))
        return fail(DVBS2_EINVAL, "nfft must be a power of two in 64..8192, hop in 1..2^24, avg not negative, n_in in 0..2^24");
    return DVBS2_OK;
}

int dvbs2_spectrum_window(int kind, int nfft, float* out)
{
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    if (spectrum_window(kind, nfft, out)) return fail(DVBS2_EINVAL, "kind must be in 0..3, nfft a power of two in 64..8192");
    return DVBS2_OK;
}

int dvbs2_spectrum_twiddles(int nfft, float* out)
{
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    if (spectrum_twiddles(nfft, out)) return fail(DVBS2_EINVAL, "nfft must be a power of two in 64..8192");
    return DVBS2_OK;
}

int dvbs2_spectrum_check(int nfft, int hop, int avg, const float* window, int max_streams, int max_samples)
{
    const std::string bad = SpectrumHip::check_args(nfft, hop, avg, window, max_streams, max_samples);
    return bad.empty() ? DVBS2_OK : fail(DVBS2_EINVAL, bad);
}

int dvbs2_spectrum_carriers(const float* psd, int nfft, int shifted, const dvbs2_spectrum_carrier_params_t* params,
                            dvbs2_spectrum_carrier_t* out, int max_out, int* n_found)
{
    API_TRY
    SpectrumCarrierParams p = kSpectrumCarrierDefaults;
    if (params) std::memcpy(&p, params, sizeof p);
    if (max_out < 0) return fail(DVBS2_EINVAL, "max_out is negative");
    if (max_out > 0 && !out) return fail(DVBS2_EINVAL, "out is null");
    if (!n_found) return fail(DVBS2_EINVAL, "n_found is null");
    const std::string bad = spectrum_carriers_check(psd, nfft, p);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    const std::vector<SpectrumCarrier> found = spectrum_carriers(psd, nfft, shifted != 0, p);
    const size_t fits = std::min(found.size(), (size_t)max_out);
    if (fits) std::memcpy(out, found.data(), fits * sizeof(SpectrumCarrier));
    *n_found = (int)found.size();
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_spectrum_create(dvbs2_spectrum_t** h, int nfft, int hop, int avg, const float* window, int shifted, int max_streams, int max_samples,
                          int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (int rc = dvbs2_spectrum_check(nfft, hop, avg, window, max_streams, max_samples)) return rc;
    return make_handle(h, device, [&] { return new (std::nothrow) SpectrumHip(nfft, hop, avg, window, shifted, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_spectrum_destroy(dvbs2_spectrum_t* h) { destroy_handle(h); }

int dvbs2_spectrum_params(const dvbs2_spectrum_t* h, int* nfft, int* hop, int* avg, int* shifted, double* window_power)
{
    NEED_HANDLE(h);
    if (nfft) *nfft = h->impl->nfft();
    if (hop) *hop = h->impl->hop();
    if (avg) *avg = h->impl->avg();
    if (shifted) *shifted = h->impl->shifted();
    if (window_power) *window_power = h->impl->window_power();
    return DVBS2_OK;
}

int dvbs2_spectrum_process_device(dvbs2_spectrum_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out,
                                  int64_t out_stride, int* n_rows_host, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int n_rows;
    if (int rc = spectrum_check_call(h, d_in, in_stride, n_in, n_streams, d_out, out_stride, &n_rows, &done)) return rc;
    if (!done) {
        if ((uintptr_t)d_in & 7) return fail(DVBS2_EINVAL, "in must be 8-byte aligned");
        if ((uintptr_t)d_out & 3) return fail(DVBS2_EINVAL, "out must be 4-byte aligned");
        if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, (hipStream_t)stream))) return rc;
    }
    if (n_rows_host) *n_rows_host = n_rows;
    return DVBS2_OK;
    API_CATCH
}

// host entry: stage the n_streams streams, run, copy the rows back
int dvbs2_spectrum_process(dvbs2_spectrum_t* h, const float* in, int64_t in_stride, int n_in, int n_streams, float* out, int64_t out_stride,
                           int* n_rows_host)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int n_rows;
    if (int rc = spectrum_check_call(h, in, in_stride, n_in, n_streams, out, out_stride, &n_rows, &done)) return rc;
    if (done) {
        if (n_rows_host) *n_rows_host = n_rows;
        return DVBS2_OK;
    }
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    if (n_streams == 1) in_stride = n_in; // (one stream: the stride does not matter)
    const size_t row_floats = (size_t)n_rows * h->impl->nfft();
    const size_t ib = ((size_t)(n_streams - 1) * in_stride + n_in) * 8, ob = ((size_t)(n_streams - 1) * out_stride + row_floats) * 4;
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, ob)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, in, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, s.stream))) return rc;
    HCHK(hipMemcpy2DAsync(out, (size_t)out_stride * 4, d_out, (size_t)out_stride * 4, row_floats * 4, (size_t)n_streams, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_rows_host) *n_rows_host = n_rows;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
