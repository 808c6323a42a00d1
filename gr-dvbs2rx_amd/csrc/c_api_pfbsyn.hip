// c_api_pfbsyn.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the polyphase synthesis filter bank, the rows of M equally spaced
// channels merged into one wideband stream, for a batch of streams.
#include <algorithm>
#include "c_api_common.h"
#include "pfbsyn_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ polyphase synthesizer */
struct dvbs2_pfbsyn {
    PfbsynHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kPfbsynSpan == DVBS2_PFBSYN_SPAN && kPfbsynSpanLong == DVBS2_PFBSYN_SPAN_LONG && kPfbsynMaxTile == DVBS2_PFBSYN_MAX_TILE &&
                  kPfbsynMaxProduct == DVBS2_PFBSYN_MAX_PRODUCT,
              "the header names the kernel's tile rule");

// the checks the work entries share, alignment apart; *done: no launch (n_in == 0, or no stream)
static int pfbsyn_check(const dvbs2_pfbsyn_t* h, const void* in, int64_t in_stride, int n_in, int n_streams, const void* out, int64_t out_stride,
                        int64_t* n_out, bool* done)
{
    const PfbsynHip& p = *h->impl;
    if (int rc = check_stream_call(h, in, n_in, "n_in", "max_samples", n_streams, out, done)) return rc;
    *n_out = p.produce(n_in);
    if (*n_out < 0) return fail(DVBS2_EINVAL, "the sample counter is exhausted");
    if (*done) return DVBS2_OK;
    if (in == out) return fail(DVBS2_EINVAL, "in and out must not be the same buffer");
    if ((size_t)n_streams * p.channels().size() > 1 && in_stride < n_in) return fail(DVBS2_EINVAL, "in_stride is below n_in");
    if (out_stride < *n_out) return fail(DVBS2_EINVAL, "out_stride is below n_out");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_pfbsyn_geometry(int n_chan, int interp, int ntaps, int* tail, int* delay_num, int* taps_per_phase)
{
    if (pfbsyn_geometry(n_chan, interp, ntaps, tail, delay_num, taps_per_phase))
        return fail(DVBS2_EINVAL, "n_chan must be a power of two in 2..256, interp in 1..n_chan, ntaps in 1..4096");
    return DVBS2_OK;
}

int dvbs2_pfbsyn_tile(int n_chan, int interp, int ntaps)
{
    if (pfbsyn_geometry(n_chan, interp, ntaps, nullptr, nullptr, nullptr))
        return fail(DVBS2_EINVAL, "n_chan must be a power of two in 2..256, interp in 1..n_chan, ntaps in 1..4096");
    if (n_chan * ((ntaps + interp - 1) / interp) > kPfbsynMaxProduct) return fail(DVBS2_EINVAL, "n_chan * ceil(ntaps / interp) must not exceed 8192");
    return pfbsyn_tile(n_chan, interp, ntaps);
}

int dvbs2_pfbsyn_check(int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples)
{
    const std::string bad = PfbsynHip::check_args(n_chan, interp, taps, ntaps, max_streams, max_samples);
    return bad.empty() ? DVBS2_OK : fail(DVBS2_EINVAL, bad);
}

int dvbs2_pfbsyn_create(dvbs2_pfbsyn_t** h, int n_chan, int interp, const float* taps, int ntaps, int max_streams, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (int rc = dvbs2_pfbsyn_check(n_chan, interp, taps, ntaps, max_streams, max_samples)) return rc;
    return make_handle(h, device, [&] { return new (std::nothrow) PfbsynHip(n_chan, interp, taps, ntaps, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_pfbsyn_destroy(dvbs2_pfbsyn_t* h) { destroy_handle(h); }

int dvbs2_pfbsyn_reset(dvbs2_pfbsyn_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_pfbsyn_set_channels(dvbs2_pfbsyn_t* h, const int* list, int n_sel)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_channels(list, n_sel));
    API_CATCH
}

int dvbs2_pfbsyn_params(const dvbs2_pfbsyn_t* h, int* n_chan, int* interp, int* ntaps, int* tail, int* delay_num, int* tile)
{
    NEED_HANDLE(h);
    if (n_chan) *n_chan = h->impl->n_chan();
    if (interp) *interp = h->impl->interp();
    if (ntaps) *ntaps = h->impl->ntaps();
    if (tail) *tail = h->impl->tail();
    if (delay_num) *delay_num = h->impl->ntaps() - 1;
    if (tile) *tile = h->impl->tile();
    return DVBS2_OK;
}

int dvbs2_pfbsyn_position(const dvbs2_pfbsyn_t* h, int64_t* counter)
{
    NEED_HANDLE(h);
    if (!counter) return fail(DVBS2_EINVAL, "counter is null");
    *counter = h->impl->position();
    return DVBS2_OK;
}

int dvbs2_pfbsyn_channels(const dvbs2_pfbsyn_t* h, int* list, int* n_sel)
{
    NEED_HANDLE(h);
    const std::vector<int32_t>& sel = h->impl->channels();
    if (list) std::copy(sel.begin(), sel.end(), list);
    if (n_sel) *n_sel = (int)sel.size();
    return DVBS2_OK;
}

int dvbs2_pfbsyn_process_device(dvbs2_pfbsyn_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride,
                                int64_t* n_out_host, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int64_t n_out;
    if (int rc = pfbsyn_check(h, d_in, in_stride, n_in, n_streams, d_out, out_stride, &n_out, &done)) return rc;
    if (!done && check_aligned8(d_in, d_out)) return DVBS2_EINVAL;
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, (hipStream_t)stream))) return rc;
    if (n_out_host) *n_out_host = n_out;
    return DVBS2_OK;
    API_CATCH
}

// host entry: stage the n_streams n_sel rows, run, copy the n_streams streams back
int dvbs2_pfbsyn_process(dvbs2_pfbsyn_t* h, const float* in, int64_t in_stride, int n_in, int n_streams, float* out, int64_t out_stride,
                         int64_t* n_out_host)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int64_t n;
    if (int rc = pfbsyn_check(h, in, in_stride, n_in, n_streams, out, out_stride, &n, &done)) return rc;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    if (done) { // (no launch: the counter of a call without streams still advances)
        if (int rc = impl_rc(h, h->impl->process_device(nullptr, 0, n_in, n_streams, nullptr, 0, s.stream))) return rc;
        if (n_out_host) *n_out_host = n;
        return DVBS2_OK;
    }
    const size_t rows = (size_t)n_streams * h->impl->channels().size();
    if (rows == 1) in_stride = n_in; // (one row: the stride does not matter)
    if (n_streams == 1) out_stride = n;
    const size_t ib = ((rows - 1) * in_stride + n_in) * 8, ob = ((size_t)(n_streams - 1) * out_stride + n) * 8;
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, ob)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, in, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, s.stream))) return rc;
    HCHK(hipMemcpy2DAsync(out, (size_t)out_stride * 8, d_out, (size_t)out_stride * 8, (size_t)n * 8, (size_t)n_streams, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_out_host) *n_out_host = n;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
