// c_api_plcoarse.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the coarse frequency estimate.
#include "c_api_common.h"
#include "plcoarse_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ coarse frequency offset estimate */
struct dvbs2_plcoarse {
    PlCoarseHip* impl = nullptr;
    HostStage stage; enum { HDR, PLSC, OUT, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    int device = 0;
};

struct dvbs2_plcoarse_batch {
    PlCoarseBatchHip* impl = nullptr;
    HostStage stage; // (no host-buffer entry: nothing is staged)
    int device = 0;
};

static PlCoarseOut plcoarse_out(float* foffset, int32_t* corrected, int32_t* new_est)
{
    PlCoarseOut o;
    o.foffset = foffset; o.corrected = corrected; o.new_est = new_est;
    return o;
}

extern "C" {

int dvbs2_plcoarse_weights(int full, float* w)
{
    if (!w) return fail(DVBS2_EINVAL, "bad argument");
    return plcoarse_weights(full, w);
}

int dvbs2_plcoarse_create(dvbs2_plcoarse_t** h, int period, int plsc_or_minus1, int max_frames, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (period < 1) return fail(DVBS2_EINVAL, "period must be at least 1");
    if (plsc_or_minus1 < -1 || plsc_or_minus1 > 127) return fail(DVBS2_EINVAL, "plsc out of range (-1 = not known, 0..127)");
    if (max_frames < 1 || max_frames > (1 << 20)) return fail(DVBS2_EINVAL, "max_frames out of range (1..1048576)");
    return make_handle(h, device, [&] { return new (std::nothrow) PlCoarseHip(period, plsc_or_minus1, max_frames, device); });
    API_CATCH
}

void dvbs2_plcoarse_destroy(dvbs2_plcoarse_t* h) { destroy_handle(h); }

int dvbs2_plcoarse_reset(dvbs2_plcoarse_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_plcoarse_estimate_device(dvbs2_plcoarse_t* h, const float* d_plframes, int64_t stride_syms, const uint8_t* d_plsc, int n_frames,
                                   float* d_coarse_foffset, int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_plframes)) return rc;
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!d_plsc && h->impl->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array");
    return impl_rc(h, h->impl->frames_device(d_plframes, stride_syms, d_plsc, n_frames, plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est),
                                             (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plcoarse_estimate_records_device(dvbs2_plcoarse_t* h, const float* d_syms, int n_syms, int64_t base_index,
                                           const dvbs2_plsync_frame_t* d_frames, int n_frames, float* d_coarse_foffset,
                                           int32_t* d_coarse_corrected, int32_t* d_new_est, void* stream)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, d_frames)) return rc;
    if (n_syms < 0 || (n_frames && !d_syms)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->records_device(d_syms, n_syms, reinterpret_cast<const PlSyncFrame*>(d_frames), n_frames, base_index,
                                              plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est), (hipStream_t)stream));
    API_CATCH
}

// host entry: stage the 90 header symbols of every frame, run, copy back what the caller asked for
int dvbs2_plcoarse_estimate(dvbs2_plcoarse_t* h, const float* plframes, int64_t stride_syms, const uint8_t* plsc, int n_frames,
                            float* coarse_foffset, int32_t* coarse_corrected, int32_t* new_est)
{
    API_TRY
    if (int rc = check_frames(h, n_frames, plframes)) return rc;
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!plsc && h->impl->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-frame PLSC array");
    if (n_frames == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t mf = h->impl->max_frames(), nf = n_frames;
    if (s.ensure(h->HDR, mf * 90 * 8) || s.ensure(h->PLSC, mf) || s.ensure(h->OUT, mf * 3 * 4)) return DVBS2_EDEVICE;
    float* d_hdr = s.at<float>(h->HDR); uint8_t* d_plsc = s.at<uint8_t>(h->PLSC);
    float* d_fo = s.at<float>(h->OUT); int32_t* d_cc = s.at<int32_t>(h->OUT) + mf; int32_t* d_ne = s.at<int32_t>(h->OUT) + 2 * mf;
    HCHK(hipMemcpy2DAsync(d_hdr, 90 * 8, plframes, (size_t)stride_syms * 8, 90 * 8, nf, hipMemcpyHostToDevice, s.stream));
    if (plsc) HCHK(hipMemcpyAsync(d_plsc, plsc, nf, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->frames_device(d_hdr, 90, plsc ? d_plsc : nullptr, n_frames, plcoarse_out(d_fo, d_cc, d_ne), s.stream))) return rc;
    if (coarse_foffset) HCHK(hipMemcpyAsync(coarse_foffset, d_fo, nf * 4, hipMemcpyDeviceToHost, s.stream));
    if (coarse_corrected) HCHK(hipMemcpyAsync(coarse_corrected, d_cc, nf * 4, hipMemcpyDeviceToHost, s.stream));
    if (new_est) HCHK(hipMemcpyAsync(new_est, d_ne, nf * 4, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

/* ------------------------------------------------------------------ the same estimate over the slots of a batch of streams */
int dvbs2_plcoarse_batch_create(dvbs2_plcoarse_batch_t** h, int period, int plsc_or_minus1, int max_streams, int max_slots, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (const std::string bad = plcoarse_batch_check(period, plsc_or_minus1, max_streams, max_slots); !bad.empty()) return fail(DVBS2_EINVAL, bad);
    return make_handle(h, device, [&] { return new (std::nothrow) PlCoarseBatchHip(period, plsc_or_minus1, max_streams, max_slots, device); });
    API_CATCH
}

void dvbs2_plcoarse_batch_destroy(dvbs2_plcoarse_batch_t* h) { destroy_handle(h); }

int dvbs2_plcoarse_batch_reset(dvbs2_plcoarse_batch_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_plcoarse_batch_reset_stream(dvbs2_plcoarse_batch_t* h, int stream_index)
{
    API_TRY
    NEED_HANDLE(h);
    if (stream_index < 0 || stream_index >= h->impl->max_streams()) return fail(DVBS2_EINVAL, "stream index out of range");
    return impl_rc(h, h->impl->reset_stream(stream_index));
    API_CATCH
}

int dvbs2_plcoarse_batch_estimate_device(dvbs2_plcoarse_batch_t* h, const float* d_slots, int64_t stride_syms, const uint8_t* d_plsc,
                                         const int32_t* d_offsets, int n_streams, float* d_coarse_foffset, int32_t* d_coarse_corrected,
                                         int32_t* d_new_est, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (int rc = check_counts({ { n_streams, h->impl->max_streams(), "n_streams", "max_streams" } })) return rc;
    if (n_streams && (!d_slots || !d_offsets)) return fail(DVBS2_EINVAL, "bad argument");
    if (stride_syms < 90) return fail(DVBS2_EINVAL, "stride below the 90 header symbols");
    if (!d_plsc && h->impl->fixed_plsc() < 0) return fail(DVBS2_EINVAL, "a handle without a fixed PLSC needs the per-slot PLSC array");
    return impl_rc(h, h->impl->slots_device(d_slots, stride_syms, d_plsc, d_offsets, n_streams, plcoarse_out(d_coarse_foffset, d_coarse_corrected, d_new_est),
                                            (hipStream_t)stream));
    API_CATCH
}

} // extern "C"
