// c_api_bbframer.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): BB framing, with the BBHEADER and CRC-8 helpers.
#include "c_api_common.h"
#include "fec_tables.h"
#include "bbframer_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ BB framing */
struct dvbs2_bbframer {
    BbFramerHip* impl = nullptr;
    HostStage stage; enum { IN, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

extern "C" {

int dvbs2_bbframer_create_raw(dvbs2_bbframer_t** h, int kbch_bits, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    const std::string bad = bbframer_check_create(kbch_bits, max_frames);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) BbFramerHip(kbch_bits, max_frames, device); });
    API_CATCH
}

int dvbs2_bbframer_create(dvbs2_bbframer_t** h, int standard, int framesize, int rate, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return dvbs2_bbframer_create_raw(h, (int)fi.bch_k, max_frames, device);
    API_CATCH
}

void dvbs2_bbframer_destroy(dvbs2_bbframer_t* h) { destroy_handle(h); }

int dvbs2_bbframer_params(const dvbs2_bbframer_t* h, int* kbch_bytes, int* max_dfl_bytes, int* max_packets_per_call)
{
    NEED_HANDLE(h);
    if (kbch_bytes) *kbch_bytes = h->impl->kbch_bytes();
    if (max_dfl_bytes) *max_dfl_bytes = h->impl->max_dfl_bytes();
    if (max_packets_per_call) *max_packets_per_call = h->impl->max_packets_per_call();
    return DVBS2_OK;
}

int dvbs2_bbframer_set_matype(dvbs2_bbframer_t* h, int matype1, int matype2)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_matype(matype1, matype2));
    API_CATCH
}

int dvbs2_bbframer_need(const dvbs2_bbframer_t* h, int n_frames, int dfl_bytes, int* n_packets)
{
    API_TRY
    NEED_HANDLE(h);
    if (!n_packets) return fail(DVBS2_EINVAL, "n_packets is null");
    return impl_rc(h, h->impl->need(n_frames, dfl_bytes, n_packets));
    API_CATCH
}

int dvbs2_bbframer_process_device(dvbs2_bbframer_t* h, const uint8_t* d_ts, int n_frames, int dfl_bytes, uint8_t* d_bbframes, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->process_device(d_ts, n_frames, dfl_bytes, d_bbframes, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbframer_process(dvbs2_bbframer_t* h, const uint8_t* ts, int n_frames, int dfl_bytes, uint8_t* bbframes, int* n_packets_read)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_packets_read) *n_packets_read = 0;
    int n_pkts = 0;
    if (int rc = impl_rc(h, h->impl->need(n_frames, dfl_bytes, &n_pkts))) return rc;
    if (n_frames == 0) return DVBS2_OK;
    if (!ts) return fail(DVBS2_EINVAL, "ts is null");
    if (!bbframes) return fail(DVBS2_EINVAL, "bbframes is null");
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t ib = (size_t)n_pkts * kBbfTsLen, ob = (size_t)n_frames * h->impl->kbch_bytes();
    if (s.ensure(h->IN, ib) || s.ensure(h->OUT, ob)) return DVBS2_EDEVICE;
    uint8_t* d_in = s.at<uint8_t>(h->IN); uint8_t* d_out = s.at<uint8_t>(h->OUT);
    HCHK(hipMemcpyAsync(d_in, ts, ib, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->process_device(d_in, n_frames, dfl_bytes, d_out, s.stream))) return rc;
    HCHK(hipMemcpyAsync(bbframes, d_out, ob, hipMemcpyDeviceToHost, s.stream));
    if (int rc = s.sync()) return rc;
    if (n_packets_read) *n_packets_read = n_pkts;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbframer_counters(dvbs2_bbframer_t* h, dvbs2_bbframer_counters_t* out, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    BbfCounters c;
    if (int rc = impl_rc(h, h->impl->counters(&c, (hipStream_t)stream))) return rc;
    out->packets = c.packets; out->bbframes = c.bbframes; out->sync_errors = c.sync_errors;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbframer_reset(dvbs2_bbframer_t* h, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset((hipStream_t)stream));
    API_CATCH
}

int dvbs2_bbheader_build(uint8_t out[10], int matype1, int matype2, int upl_bits, int dfl_bits, int sync, int syncd_bits)
{
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    if (bbheader_build(out, matype1, matype2, upl_bits, dfl_bits, sync, syncd_bits))
        return fail(DVBS2_EINVAL, "matype1, matype2 and sync must be in 0..255, upl_bits, dfl_bits and syncd_bits in 0..65535");
    return DVBS2_OK;
}

int dvbs2_crc8(const uint8_t* data, size_t n)
{
    if (!data && n) return fail(DVBS2_EINVAL, "data is null");
    return crc8(data, n);
}

} // extern "C"
