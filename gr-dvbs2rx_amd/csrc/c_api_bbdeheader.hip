// c_api_bbdeheader.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the BBFRAME de-header.
#include "c_api_common.h"
#include "fec_tables.h"
#include "bbdeheader_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ BBFRAME de-header */
struct dvbs2_bbdeheader {
    BbDeheaderHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

extern "C" {

int dvbs2_bbdeheader_create_raw(dvbs2_bbdeheader_t** h, int kbch_bits, int max_frames, int device)
{
    API_TRY
    return make_handle(h, device, [&] { return new (std::nothrow) BbDeheaderHip(kbch_bits, max_frames, device); });
    API_CATCH
}

int dvbs2_bbdeheader_create(dvbs2_bbdeheader_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return dvbs2_bbdeheader_create_raw(h, (int)fi.bch_k, max_frames, device); // d_kbch_bytes, d_max_dfl (:58-61)
    API_CATCH
}

void dvbs2_bbdeheader_destroy(dvbs2_bbdeheader_t* h) { destroy_handle(h); }

int dvbs2_bbdeheader_params(const dvbs2_bbdeheader_t* h, int* kbch_bytes, int* max_dfl_bits, int* max_out_bytes_per_frame)
{
    NEED_HANDLE(h);
    if (kbch_bytes) *kbch_bytes = h->impl->kbch_bytes();
    if (max_dfl_bits) *max_dfl_bits = h->impl->max_dfl();
    if (max_out_bytes_per_frame) *max_out_bytes_per_frame = h->impl->max_out_bytes_per_frame();
    return DVBS2_OK;
}

int dvbs2_bbdeheader_process_device(dvbs2_bbdeheader_t* h, const uint8_t* d_bbframes, int n_frames, uint8_t* d_ts_out, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_bbframes && d_ts_out)) return rc;
    return impl_rc(h, h->impl->process_device(d_bbframes, n_frames, d_ts_out, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbdeheader_finish(dvbs2_bbdeheader_t* h, int64_t* produced, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    BbdhState st;
    if (int rc = impl_rc(h, h->impl->state(&st, (hipStream_t)stream))) return rc;
    if (produced) *produced = (int64_t)st.produced;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_counters(dvbs2_bbdeheader_t* h, dvbs2_bbdeheader_counters_t* out, void* stream)
{
    API_TRY
    if (!h || !out) return fail(DVBS2_EINVAL, "bad argument");
    BbdhState st;
    if (int rc = impl_rc(h, h->impl->state(&st, (hipStream_t)stream))) return rc;
    out->packets = st.packets; out->errors = st.errors; out->bbframes = st.bbframes; out->dropped = st.dropped; out->gaps = st.gaps;
    out->overruns = st.overruns; out->synched = st.synched; out->partial_ts_bytes = st.partial;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_reset(dvbs2_bbdeheader_t* h, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset((hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbdeheader_process(dvbs2_bbdeheader_t* h, const uint8_t* bbframes, int n_frames, uint8_t* ts_out, int64_t* produced)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, bbframes && ts_out)) return rc;
    if (produced) *produced = 0;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = h->impl->max_frames(), fb = h->impl->kbch_bytes(), ob = h->impl->max_out_bytes_per_frame();
    if (s.ensure(h->IN, mf * fb) || s.ensure(h->OUT, mf * ob)) return DVBS2_EDEVICE;
    uint8_t* d_in = s.at<uint8_t>(h->IN); uint8_t* d_out = s.at<uint8_t>(h->OUT);
    if (n_frames) HCHK(hipMemcpyAsync(d_in, bbframes, (size_t)n_frames * fb, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, n_frames, d_out, s.stream))) return rc;
    BbdhState st;
    if (int rc = impl_rc(h, h->impl->state(&st, s.stream))) return rc;
    if (st.produced > 0) {
        HCHK(hipMemcpyAsync(ts_out, d_out, (size_t)st.produced, hipMemcpyDeviceToHost, s.stream));
        if (int rc = s.sync()) return rc;
    }
    if (produced) *produced = (int64_t)st.produced;
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
