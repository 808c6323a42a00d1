// c_api_plframer.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the PL framer of the forward direction.
#include "c_api_common.h"
#include "plframer_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ PL framer: XFECFRAMEs -> PLFRAMEs (PLHEADER, pilots, PL scrambling) */
struct dvbs2_plframer {
    PlFramerHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

// the checks the two framing entries share; buffers are checked for n_frames > 0 only, the input only where a data frame reads it
static int plframer_check(const dvbs2_plframer* h, const void* xfecframes, int n_frames, int closing_plsc, const void* plframes)
{
    NEED_HANDLE(h);
    if (n_frames < 0) return fail(DVBS2_EINVAL, "n_frames is negative");
    if (closing_plsc < -1 || closing_plsc > 127) return fail(DVBS2_EINVAL, "closing_plsc out of range (-1 = none, 0..127)");
    if (closing_plsc >= 0) if (const char* why = plframer_refusal(closing_plsc)) return fail(DVBS2_EINVAL, std::string("closing_plsc ") + why);
    if (n_frames > h->impl->n_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds the sequence");
    if (n_frames && !plframes) return fail(DVBS2_EINVAL, "plframes is null");
    if (n_frames && !xfecframes && h->impl->in_end(n_frames) > 0) return fail(DVBS2_EINVAL, "xfecframes is null and the framed prefix holds a data frame");
    return DVBS2_OK;
}

extern "C" {

int dvbs2_plframer_layout(const uint8_t* plsc, int n_frames, int64_t* in_offset, int64_t* out_offset, int64_t* in_syms, int64_t* out_syms)
{
    API_TRY
    if (n_frames < 0 || (n_frames && !plsc)) return fail(DVBS2_EINVAL, "bad argument");
    std::vector<PlFramerRec> rec(n_frames);
    std::string why;
    if (!plframer_layout(plsc, n_frames, rec.data(), in_syms, out_syms, &why)) return fail(DVBS2_EINVAL, why);
    for (int f = 0; f < n_frames; f++) {
        if (in_offset) in_offset[f] = rec[f].in_offset;
        if (out_offset) out_offset[f] = rec[f].out_offset;
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_plframer_create(dvbs2_plframer_t** h, int gold_code, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, [&] { return new (std::nothrow) PlFramerHip(gold_code, max_frames, device); });
    API_CATCH
}

void dvbs2_plframer_destroy(dvbs2_plframer_t* h) { destroy_handle(h); }

int dvbs2_plframer_set_sequence(dvbs2_plframer_t* h, const uint8_t* plsc, int n_frames)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_frames < 0 || (n_frames && !plsc)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->set_sequence(plsc, n_frames));
    API_CATCH
}

int dvbs2_plframer_params(const dvbs2_plframer_t* h, int* n_frames, int64_t* in_syms, int64_t* out_syms)
{
    NEED_HANDLE(h);
    if (n_frames) *n_frames = h->impl->n_frames();
    if (in_syms) *in_syms = h->impl->in_syms();
    if (out_syms) *out_syms = h->impl->out_syms();
    return DVBS2_OK;
}

int dvbs2_plframer_frame_device(dvbs2_plframer_t* h, const float* d_xfecframes, int n_frames, int closing_plsc, float* d_plframes, void* stream)
{
    API_TRY
    if (int rc = plframer_check(h, d_xfecframes, n_frames, closing_plsc, d_plframes)) return rc;
    return impl_rc(h, h->impl->frame_device(d_xfecframes, n_frames, closing_plsc, d_plframes, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plframer_frame(dvbs2_plframer_t* h, const float* xfecframes, int n_frames, int closing_plsc, float* plframes)
{
    API_TRY
    if (int rc = plframer_check(h, xfecframes, n_frames, closing_plsc, plframes)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    // sized for the sequence as it is set: the buffers grow when a longer one follows
    const size_t in_bytes = (size_t)h->impl->in_end(n_frames) * 8, out_bytes = ((size_t)h->impl->out_end(n_frames) + (closing_plsc >= 0 ? 90 : 0)) * 8;
    if (s.ensure(h->IN, (size_t)h->impl->in_syms() * 8 + 16) || s.ensure(h->OUT, ((size_t)h->impl->out_syms() + 90) * 8)) return DVBS2_EDEVICE;
    float* d_in = s.at<float>(h->IN); float* d_out = s.at<float>(h->OUT);
    if (in_bytes) HCHK(hipMemcpyAsync(d_in, xfecframes, in_bytes, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->frame_device(d_in, n_frames, closing_plsc, d_out, s.stream))) return rc;
    HCHK(hipMemcpyAsync(plframes, d_out, out_bytes, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
