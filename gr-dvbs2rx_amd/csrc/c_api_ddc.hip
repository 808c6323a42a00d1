// c_api_ddc.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): digital down-conversion, a frequency-translating decimating FIR over a
// batch of channels.
#include <algorithm>
#include "c_api_common.h"
#include "ddc_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ digital down-conversion */
struct dvbs2_ddc {
    DdcHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kDdcSpan == DVBS2_DDC_SPAN && kDdcMaxTile == DVBS2_DDC_MAX_TILE, "the header names the kernel's tile rule");

// the checks the work entries share, buffers and alignment apart; *done: no launch (n_in == 0, or no channel)
static int ddc_check(const dvbs2_ddc_t* h, const void* in, int64_t in_stride, int n_in, int n_inputs, int n_channels, const void* out,
                     int64_t out_stride, int64_t* n_out, bool* done)
{
    const DdcHip& d = *h->impl;
    *done = false;
    if (int rc = check_counts({ { n_in, d.max_samples(), "n_in", "max_samples" }, { n_inputs, d.max_inputs(), "n_inputs", "max_inputs" },
                                { n_channels, d.max_channels(), "n_channels", "max_channels" } })) return rc;
    *n_out = d.produce(n_in);
    if (*n_out < 0) return fail(DVBS2_EINVAL, "the sample counter is exhausted");
    if (n_in == 0 || n_channels == 0) { *done = true; return DVBS2_OK; }
    if (int rc = check_in_out(in, out)) return rc;
    for (int c = 0; c < n_channels; c++)
        if (d.input_of(c) >= n_inputs) return fail(DVBS2_EINVAL, "channel " + std::to_string(c) + " reads input " + std::to_string(d.input_of(c)) + ", which is not below n_inputs");
    if (n_inputs > 1 && in_stride < n_in) return fail(DVBS2_EINVAL, "in_stride is below n_in");
    if (out_stride < *n_out) return fail(DVBS2_EINVAL, "out_stride is below n_out");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_ddc_geometry(int decim, int ntaps, int* history, int* delay_num)
{
    if (ddc_geometry(decim, ntaps, history, delay_num)) return fail(DVBS2_EINVAL, "decim must be in 1..256, ntaps in 1..4096");
    return DVBS2_OK;
}

int64_t dvbs2_ddc_produce(int64_t position, int decim, int n_in)
{
    const int64_t n = ddc_produce(position, decim, n_in);
    if (n < 0) return fail(DVBS2_EINVAL, "position must be in 0..2^62, decim in 1..256, n_in in 0..2^24");
    return n;
}

int dvbs2_ddc_check(int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples)
{
    const std::string bad = DdcHip::check_args(decim, taps, ntaps, max_channels, max_inputs, max_samples);
    return bad.empty() ? DVBS2_OK : fail(DVBS2_EINVAL, bad);
}

int dvbs2_ddc_create(dvbs2_ddc_t** h, int decim, const float* taps, int ntaps, int max_channels, int max_inputs, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (int rc = dvbs2_ddc_check(decim, taps, ntaps, max_channels, max_inputs, max_samples)) return rc;
    return make_handle(h, device, [&] { return new (std::nothrow) DdcHip(decim, taps, ntaps, max_channels, max_inputs, max_samples, device); });
    API_CATCH
}

void dvbs2_ddc_destroy(dvbs2_ddc_t* h) { destroy_handle(h); }

int dvbs2_ddc_reset(dvbs2_ddc_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_ddc_set_channel(dvbs2_ddc_t* h, int channel, int input, double phase_inc)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_channel(channel, input, phase_inc));
    API_CATCH
}

int dvbs2_ddc_params(const dvbs2_ddc_t* h, int* decim, int* ntaps, int* history, int* delay_num, int* tile)
{
    NEED_HANDLE(h);
    if (decim) *decim = h->impl->decim();
    if (ntaps) *ntaps = h->impl->ntaps();
    if (history) *history = h->impl->history();
    if (delay_num) *delay_num = h->impl->ntaps() - 1;
    if (tile) *tile = h->impl->tile();
    return DVBS2_OK;
}

int dvbs2_ddc_position(const dvbs2_ddc_t* h, int64_t* counter)
{
    NEED_HANDLE(h);
    if (!counter) return fail(DVBS2_EINVAL, "counter is null");
    *counter = h->impl->mirror().counter;
    return DVBS2_OK;
}

int dvbs2_ddc_channel(const dvbs2_ddc_t* h, int channel, int* input, uint64_t* inc_turns, uint64_t* phase_turns)
{
    NEED_HANDLE(h);
    if (channel < 0 || channel >= h->impl->max_channels()) return fail(DVBS2_EINVAL, "channel out of range");
    if (input) *input = h->impl->input_of(channel);
    if (inc_turns) *inc_turns = h->impl->mirror().inc[channel];
    if (phase_turns) *phase_turns = h->impl->mirror().phase[channel];
    return DVBS2_OK;
}

int dvbs2_ddc_state(dvbs2_ddc_t* h, uint64_t* phases)
{
    API_TRY
    NEED_HANDLE(h);
    if (!phases) return fail(DVBS2_EINVAL, "phases is null");
    return impl_rc(h, h->impl->state(phases));
    API_CATCH
}

int dvbs2_ddc_process_device(dvbs2_ddc_t* h, const float* d_in, int64_t in_stride, int n_in, int n_inputs, int n_channels, float* d_out,
                             int64_t out_stride, int64_t* n_out_host, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int64_t n_out;
    if (int rc = ddc_check(h, d_in, in_stride, n_in, n_inputs, n_channels, d_out, out_stride, &n_out, &done)) return rc;
    if (!done && check_aligned8(d_in, d_out)) return DVBS2_EINVAL;
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_channels, d_out, out_stride, (hipStream_t)stream))) return rc;
    if (n_out_host) *n_out_host = n_out;
    return DVBS2_OK;
    API_CATCH
}

// host entry: stage the n_inputs streams, run, copy the n_channels outputs back
int dvbs2_ddc_process(dvbs2_ddc_t* h, const float* in, int64_t in_stride, int n_in, int n_inputs, int n_channels, float* out, int64_t out_stride,
                      int64_t* n_out_host)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    int64_t n;
    if (int rc = ddc_check(h, in, in_stride, n_in, n_inputs, n_channels, out, out_stride, &n, &done)) return rc;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    if (done) { // (no launch: the counter of a call without channels still advances)
        if (int rc = impl_rc(h, h->impl->process_device(nullptr, 0, n_in, n_channels, nullptr, 0, s.stream))) return rc;
        if (n_out_host) *n_out_host = n;
        return DVBS2_OK;
    }
    if (n_inputs == 1) in_stride = n_in; // (one stream: the stride does not matter)
    const size_t ib = ((size_t)(n_inputs - 1) * in_stride + n_in) * 8, ob = ((size_t)(n_channels - 1) * out_stride + n) * 8;
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, std::max(ob, (size_t)8))) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, in, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, in_stride, n_in, n_channels, d_out, out_stride, s.stream))) return rc;
    if (n) HCHK(hipMemcpy2DAsync(out, (size_t)out_stride * 8, d_out, (size_t)out_stride * 8, (size_t)n * 8, (size_t)n_channels, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_out_host) *n_out_host = n;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
