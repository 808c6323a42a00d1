// c_api_iqconv.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the IQ sample converter at the ends of both flowgraphs -- u8 / s8 /
// s16 codes to float samples and back, with the level statistics.
#include <cstdint>
#include "c_api_common.h"
#include "iqconv_hip.h"
#include "iqconv_math.hpp"

using namespace dvbs2;

struct dvbs2_iqconv {
    IqconvHip* impl = nullptr;
    HostStage stage; enum { CODES, STATS, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

static_assert(kIqconvTile == DVBS2_IQCONV_TILE, "the header names the kernel's tile");
static_assert(kIqU8 == DVBS2_IQ_U8 && kIqS8 == DVBS2_IQ_S8 && kIqS16 == DVBS2_IQ_S16, "the header names the formats");

// the checks every work entry shares: `codes` and `floats` are in and out of unpack, out and in of pack; *done: nothing to do
static int iqconv_check_call(const dvbs2_iqconv_t* h, int n_samples, int n_streams, const void* codes, const char* codes_name, int64_t code_stride,
                             const float* floats, const char* floats_name, int64_t float_stride, const uint64_t* stats, bool* done)
{
    *done = false;
    if (int rc = check_stream_counts(h, n_samples, "n_samples", "max_samples", n_streams)) return rc;
    if (n_samples == 0 || n_streams == 0) { *done = true; return DVBS2_OK; }
    const std::string cn = codes_name, fn = floats_name;
    if (!codes) return fail(DVBS2_EINVAL, cn + " is null");
    if (!floats) return fail(DVBS2_EINVAL, fn + " is null");
    if (h->impl->format() == DVBS2_IQ_S16 && ((uintptr_t)codes & 1)) return fail(DVBS2_EINVAL, cn + " must be 2-byte aligned for s16");
    if ((uintptr_t)floats & 7) return fail(DVBS2_EINVAL, fn + " must be 8-byte aligned");
    if ((uintptr_t)stats & 7) return fail(DVBS2_EINVAL, "stats must be 8-byte aligned");
    if (n_streams > 1 && code_stride < n_samples) return fail(DVBS2_EINVAL, cn + "_stride is below n_samples");
    if (n_streams > 1 && float_stride < n_samples) return fail(DVBS2_EINVAL, fn + "_stride is below n_samples");
    return DVBS2_OK;
}

// what the two host restatements share
static int iqconv_check_host(int format, float gain, const void* in, int64_t n, const void* out)
{
    const std::string bad = iqconv_check(format, gain, 1, 1);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    if (n < 0) return fail(DVBS2_EINVAL, "n is negative");
    if (n > 0 && !in) return fail(DVBS2_EINVAL, "in is null");
    if (n > 0 && !out) return fail(DVBS2_EINVAL, "out is null");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_iqconv_bytes(int format) { return iqconv_bytes(format); }

int dvbs2_iqconv_check(int format, float gain, int max_streams, int max_samples)
{
    API_TRY
    const std::string bad = iqconv_check(format, gain, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_iqconv_unpack_host(int format, float gain, const void* in, int64_t n, float* out, uint64_t* stats)
{
    API_TRY
    if (int rc = iqconv_check_host(format, gain, in, n, out)) return rc;
    iqconv_unpack_host(format, gain, in, n, out, stats);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_iqconv_pack_host(int format, float gain, const float* in, int64_t n, void* out, uint64_t* stats)
{
    API_TRY
    if (int rc = iqconv_check_host(format, gain, in, n, out)) return rc;
    iqconv_pack_host(format, gain, in, n, out, stats);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_iqconv_create(dvbs2_iqconv_t** h, int format, float gain, int max_streams, int max_samples, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = iqconv_check(format, gain, max_streams, max_samples);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) IqconvHip(format, gain, max_streams, max_samples, device); });
    API_CATCH
}

void dvbs2_iqconv_destroy(dvbs2_iqconv_t* h) { destroy_handle(h); }

int dvbs2_iqconv_set_gain(dvbs2_iqconv_t* h, float gain)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_gain(gain));
    API_CATCH
}

int dvbs2_iqconv_params(const dvbs2_iqconv_t* h, int* format, float* gain, int* max_streams, int* max_samples, int* tile)
{
    NEED_HANDLE(h);
    if (format) *format = h->impl->format();
    if (gain) *gain = h->impl->gain();
    if (max_streams) *max_streams = h->impl->max_streams();
    if (max_samples) *max_samples = h->impl->max_samples();
    if (tile) *tile = kIqconvTile;
    return DVBS2_OK;
}

int dvbs2_iqconv_unpack_device(dvbs2_iqconv_t* h, const void* d_in, int64_t in_stride, int n_samples, int n_streams, float* d_out,
                               int64_t out_stride, uint64_t* d_stats, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = iqconv_check_call(h, n_samples, n_streams, d_in, "in", in_stride, d_out, "out", out_stride, d_stats, &done)) return rc;
    if (done) return DVBS2_OK;
    return impl_rc(h, h->impl->unpack_device(d_in, in_stride, n_samples, n_streams, d_out, out_stride, d_stats, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_iqconv_pack_device(dvbs2_iqconv_t* h, const float* d_in, int64_t in_stride, int n_samples, int n_streams, void* d_out,
                             int64_t out_stride, uint64_t* d_stats, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = iqconv_check_call(h, n_samples, n_streams, d_out, "out", out_stride, d_in, "in", in_stride, d_stats, &done)) return rc;
    if (done) return DVBS2_OK;
    return impl_rc(h, h->impl->pack_device(d_in, in_stride, n_samples, n_streams, d_out, out_stride, d_stats, (hipStream_t)stream));
    API_CATCH
}

// host codes -> device floats, one row: the codes are staged, the statistics are summed in a buffer of the handle and added to the caller's
int dvbs2_iqconv_unpack_to_device(dvbs2_iqconv_t* h, const void* in, int n_samples, float* d_out, uint64_t* stats)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = iqconv_check_call(h, n_samples, 1, in, "in", n_samples, d_out, "out", n_samples, nullptr, &done)) return rc;
    if (done) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t bytes = (size_t)n_samples * iqconv_bytes(h->impl->format());
    if (s.ensure(h->CODES, bytes) || s.ensure(h->STATS, 3 * sizeof(uint64_t))) return DVBS2_EDEVICE;
    uint64_t* d_stats = stats ? s.at<uint64_t>(h->STATS) : nullptr;
    uint64_t sum[3] = {};
    HCHK(hipMemcpyAsync(s.buf[h->CODES], in, bytes, hipMemcpyHostToDevice, s.stream));
    if (stats) HCHK(hipMemsetAsync(d_stats, 0, sizeof sum, s.stream));
    if (int rc = impl_rc(h, h->impl->unpack_device(s.buf[h->CODES], n_samples, n_samples, 1, d_out, n_samples, d_stats, s.stream))) return rc;
    if (stats) HCHK(hipMemcpyAsync(sum, d_stats, sizeof sum, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (stats) for (int i = 0; i < 3; i++) stats[i] += sum[i];
    return DVBS2_OK;
    API_CATCH
}

// device floats -> host codes, one row
int dvbs2_iqconv_pack_from_device(dvbs2_iqconv_t* h, const float* d_in, int n_samples, void* out, uint64_t* stats)
{
    API_TRY
    NEED_HANDLE(h);
    bool done;
    if (int rc = iqconv_check_call(h, n_samples, 1, out, "out", n_samples, d_in, "in", n_samples, nullptr, &done)) return rc;
    if (done) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t bytes = (size_t)n_samples * iqconv_bytes(h->impl->format());
    if (s.ensure(h->CODES, bytes) || s.ensure(h->STATS, 3 * sizeof(uint64_t))) return DVBS2_EDEVICE;
    uint64_t* d_stats = stats ? s.at<uint64_t>(h->STATS) : nullptr;
    uint64_t sum[3] = {};
    if (stats) HCHK(hipMemsetAsync(d_stats, 0, sizeof sum, s.stream));
    if (int rc = impl_rc(h, h->impl->pack_device(d_in, n_samples, n_samples, 1, s.buf[h->CODES], n_samples, d_stats, s.stream))) return rc;
    HCHK(hipMemcpyAsync(out, s.buf[h->CODES], bytes, hipMemcpyDeviceToHost, s.stream));
    if (stats) HCHK(hipMemcpyAsync(sum, d_stats, sizeof sum, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (stats) for (int i = 0; i < 3; i++) stats[i] += sum[i];
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
