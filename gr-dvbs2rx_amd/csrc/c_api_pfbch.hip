// c_api_pfbch.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the polyphase filter bank channelizer, M equally spaced channels of
// a batch of streams.
#include <algorithm>
#include "c_api_common.h"
#include "pfbch_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ polyphase channelizer */
struct dvbs2_pfbch {
    PfbchHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kPfbchSpan == DVBS2_PFBCH_SPAN && kPfbchMaxTile == DVBS2_PFBCH_MAX_TILE, "the header names the kernel's tile rule");

// the checks the work entries share, alignment apart; *done: no launch (n_in == 0, or no stream)
static int pfbch_check(const dvbs2_pfbch_t* h, const void* in, int64_t in_stride, int n_in, int n_streams, const void* out, int64_t out_stride,
                       int64_t* n_out, bool* done)
{
    const PfbchHip& p = *h->impl;
    if (int rc = check_stream_call(h, in, n_in, "n_in", "max_samples", n_streams, out, done)) return rc;
    *n_out = p.produce(n_in);
    if (*n_out < 0) return fail(DVBS2_EINVAL, "the sample counter is exhausted");
    if (*done) return DVBS2_OK;
    if (in == out) return fail(DVBS2_EINVAL, "in and out must not be the same buffer");
    if (n_streams > 1 && in_stride < n_in) return fail(DVBS2_EINVAL, "in_stride is below n_in");
    if (out_stride < *n_out) return fail(DVBS2_EINVAL, "out_stride is below n_out");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_pfbch_geometry(int n_chan, int decim, int ntaps, int* history, int* delay_num, int* taps_per_branch)
{
    if (pfbch_geometry(n_chan, decim, ntaps, history, delay_num, taps_per_branch))
        return fail(DVBS2_EINVAL, "n_chan must be a power of two in 2..256, decim in 1..n_chan, ntaps in 1..4096");
    return DVBS2_OK;
}

int64_t dvbs2_pfbch_produce(int64_t position, int decim, int n_in)
{
    const int64_t n = pfbch_produce(position, decim, n_in);
    if (n < 0) return fail(DVBS2_EINVAL, "position must be in 0..2^62, decim in 1..256, n_in in 0..2^24");
    return n;
}

int dvbs2_pfbch_twiddles(int n_chan, float* out)
{
    if (pfbch_twiddles(n_chan, out)) return fail(DVBS2_EINVAL, "n_chan must be a power of two in 2..256 and out not null");
    return DVBS2_OK;
}

int dvbs2_pfbch_check(int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples)
{
    const std::string bad = PfbchHip::check_args(n_chan, decim, taps, ntaps, max_streams, max_samples);
    return bad.empty() ? DVBS2_OK : fail(DVBS2_EINVAL, bad);
}

int dvbs2_pfbch_create(dvbs2_pfbch_t** h, int n_chan, int decim, const float* taps, int ntaps, int max_streams, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (int rc = dvbs2_pfbch_check(n_chan, decim, taps, ntaps, max_streams, max_samples)) return rc;
    return make_handle(h, device, [&] { return new (std::nothrow) PfbchHip(n_chan, decim, taps, ntaps, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_pfbch_destroy(dvbs2_pfbch_t* h) { destroy_handle(h); }

int dvbs2_pfbch_reset(dvbs2_pfbch_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_pfbch_set_channels(dvbs2_pfbch_t* h, const int* list, int n_sel)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_channels(list, n_sel));
    API_CATCH
}

int dvbs2_pfbch_params(const dvbs2_pfbch_t* h, int* n_chan, int* decim, int* ntaps, int* history, int* delay_num, int* tile)
{
    NEED_HANDLE(h);
    if (n_chan) *n_chan = h->impl->n_chan();
    if (decim) *decim = h->impl->decim();
    if (ntaps) *ntaps = h->impl->ntaps();
    if (history) *history = h->impl->history();
    if (delay_num) *delay_num = h->impl->ntaps() - 1;
    if (tile) *tile = h->impl->tile();
    return DVBS2_OK;
}

int dvbs2_pfbch_position(const dvbs2_pfbch_t* h, int64_t* counter)
{
    NEED_HANDLE(h);
    if (!counter) return fail(DVBS2_EINVAL, "counter is null");
    *counter = h->impl->position();
    return DVBS2_OK;
}

int dvbs2_pfbch_channels(const dvbs2_pfbch_t* h, int* list, int* n_sel)
{
    NEED_HANDLE(h);
    const std::vector<int32_t>& sel = h->impl->channels();
    if (list) std::copy(sel.begin(), sel.end(), list);
    if (n_sel) *n_sel = (int)sel.size();
    return DVBS2_OK;
}

int dvbs2_pfbch_process_device(dvbs2_pfbch_t* h, const float* d_in, int64_t in_stride, int n_in, int n_streams, float* d_out, int64_t out_stride,
                               int64_t* n_out_host, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int64_t n_out;
    if (int rc = pfbch_check(h, d_in, in_stride, n_in, n_streams, d_out, out_stride, &n_out, &done)) return rc;
    if (!done && check_aligned8(d_in, d_out)) return DVBS2_EINVAL;
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, (hipStream_t)stream))) return rc;
    if (n_out_host) *n_out_host = n_out;
    return DVBS2_OK;
    API_CATCH
}

// host entry: stage the n_streams streams, run, copy the n_streams n_sel rows back
int dvbs2_pfbch_process(dvbs2_pfbch_t* h, const float* in, int64_t in_stride, int n_in, int n_streams, float* out, int64_t out_stride,
                        int64_t* n_out_host)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int64_t n;
    if (int rc = pfbch_check(h, in, in_stride, n_in, n_streams, out, out_stride, &n, &done)) return rc;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    if (done) { // (no launch: the counter of a call without streams still advances)
        if (int rc = impl_rc(h, h->impl->process_device(nullptr, 0, n_in, n_streams, nullptr, 0, s.stream))) return rc;
        if (n_out_host) *n_out_host = n;
        return DVBS2_OK;
    }
    if (n_streams == 1) in_stride = n_in; // (one stream: the stride does not matter)
    const size_t rows = (size_t)n_streams * h->impl->channels().size();
    const size_t ib = ((size_t)(n_streams - 1) * in_stride + n_in) * 8, ob = ((rows - 1) * out_stride + n) * 8;
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, std::max(ob, (size_t)8))) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, in, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_streams, d_out, out_stride, s.stream))) return rc;
    if (n) HCHK(hipMemcpy2DAsync(out, (size_t)out_stride * 8, d_out, (size_t)out_stride * 8, (size_t)n * 8, rows, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_out_host) *n_out_host = n;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
