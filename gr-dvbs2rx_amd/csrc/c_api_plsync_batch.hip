// c_api_plsync_batch.hip -- extern "C" boundary (include/dvbs2_fec_hip.h, the batched stages): the PLFRAME search for a batch of streams.
#include "c_api_common.h"
#include "plsync_batch_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ batched PLFRAME search: metric, one tracker per stream, gather into slots */
struct dvbs2_plsync_batch {
    PlSyncBatchHip* impl = nullptr;
    HostStage stage; // (no host-buffer entry: nothing is staged)
    int device = 0;
};

extern "C" {

int dvbs2_plsync_batch_check(int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames)
{
    const std::string bad = plsync_batch_check(plsc_or_minus1, unlock_thresh, max_streams, max_symbols, max_frames);
    return bad.empty() ? DVBS2_OK : fail(DVBS2_EINVAL, bad);
}

int dvbs2_plsync_batch_check_search(int max_streams, int max_symbols, int64_t stride_syms, const int* first, const int* n_syms, int n_streams)
{
    if (int rc = check_counts({ { n_streams, max_streams, "n_streams", "max_streams" } })) return rc;
    if (n_streams == 0) return DVBS2_OK;
    if (!first) return fail(DVBS2_EINVAL, "first is null");
    if (!n_syms) return fail(DVBS2_EINVAL, "n_syms is null");
    if (stride_syms < 0) return fail(DVBS2_EINVAL, "stride_syms is negative");
    for (int s = 0; s < n_streams; s++) {
        const std::string at = "[" + std::to_string(s) + "]";
        if (first[s] < 0) return fail(DVBS2_EINVAL, "first" + at + " is negative");
        if (n_syms[s] < 0) return fail(DVBS2_EINVAL, "n_syms" + at + " is negative");
        if (n_syms[s] > max_symbols) return fail(DVBS2_ESIZE, "n_syms" + at + " exceeds max_symbols");
        // rows of a batch must not run into each other; one row may lie anywhere
        if (n_streams > 1 && (int64_t)first[s] + n_syms[s] > stride_syms) return fail(DVBS2_EINVAL, "first" + at + " + n_syms" + at + " exceeds stride_syms");
    }
    return DVBS2_OK;
}

int dvbs2_plsync_batch_create(dvbs2_plsync_batch_t** h, int plsc_or_minus1, int unlock_thresh, int max_streams, int max_symbols, int max_frames,
                              int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    // arguments first: a bad argument is the caller's mistake on any machine
    if (int rc = dvbs2_plsync_batch_check(plsc_or_minus1, unlock_thresh, max_streams, max_symbols, max_frames)) return rc;
    return make_handle(h, device, [&] { return new (std::nothrow) PlSyncBatchHip(plsc_or_minus1, unlock_thresh, max_streams, max_symbols, max_frames, device); });
    API_CATCH
}

void dvbs2_plsync_batch_destroy(dvbs2_plsync_batch_t* h) { destroy_handle(h); }

int dvbs2_plsync_batch_reset(dvbs2_plsync_batch_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->reset());
    API_CATCH
}

int dvbs2_plsync_batch_reset_stream(dvbs2_plsync_batch_t* h, int stream_index)
{
    API_TRY
    NEED_HANDLE(h);
    if (stream_index < 0 || stream_index >= h->impl->max_streams()) return fail(DVBS2_EINVAL, "stream index out of range");
    return impl_rc(h, h->impl->reset_stream(stream_index));
    API_CATCH
}

int dvbs2_plsync_batch_set_plsc_mode(dvbs2_plsync_batch_t* h, int coherent, int soft)
{
    NEED_HANDLE(h);
    h->impl->set_plsc_mode(coherent, soft);
    return DVBS2_OK;
}

int dvbs2_plsync_batch_set_expected_pls(dvbs2_plsync_batch_t* h, const uint8_t* plsc_list, int n)
{
    API_TRY
    NEED_HANDLE(h);
    if (n < 0 || (n > 0 && !plsc_list)) return fail(DVBS2_EINVAL, "bad argument");
    return impl_rc(h, h->impl->set_expected_pls(plsc_list, n));
    API_CATCH
}

int dvbs2_plsync_batch_search_device(dvbs2_plsync_batch_t* h, const float* d_syms, int64_t stride_syms, const int* first, const int* n_syms,
                                     int n_streams, dvbs2_plsync_frame_t* d_frames, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (int rc = dvbs2_plsync_batch_check_search(h->impl->max_streams(), h->impl->max_symbols(), stride_syms, first, n_syms, n_streams)) return rc;
    if (n_streams && (!d_syms || !d_frames)) return fail(DVBS2_EINVAL, "bad argument");
    if ((uintptr_t)d_syms & 7) return fail(DVBS2_EINVAL, "d_syms must be 8-byte aligned");
    return impl_rc(h, h->impl->search_device(d_syms, stride_syms, first, n_syms, n_streams, reinterpret_cast<PlSyncFrame*>(d_frames), (hipStream_t)stream));
    API_CATCH
}

int dvbs2_plsync_batch_finish(dvbs2_plsync_batch_t* h, int* n_frames, int* consumed, int* state)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->finish(n_frames, consumed, state) < 0);
    API_CATCH
}

int dvbs2_plsync_batch_gather_device(dvbs2_plsync_batch_t* h, const float* d_syms, int64_t stride_syms, const dvbs2_plsync_frame_t* d_frames,
                                     int n_streams, int wanted_plsc, float* d_slots, int max_slots, int32_t* d_offsets, int32_t* d_slot_record,
                                     void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (wanted_plsc < 0 || wanted_plsc > 127) return fail(DVBS2_EINVAL, "plsc out of range (0..127)");
    if (int rc = check_counts({ { n_streams, h->impl->max_streams(), "n_streams", "max_streams" }, { max_slots, 1 << 24, "max_slots", "2^24" } })) return rc;
    if (!d_offsets || stride_syms < 0 || (n_streams && (!d_syms || !d_frames)) || (max_slots && !d_slots)) return fail(DVBS2_EINVAL, "bad argument");
    if (((uintptr_t)d_syms | (uintptr_t)d_slots) & 7) return fail(DVBS2_EINVAL, "d_syms and d_slots must be 8-byte aligned");
    return impl_rc(h, h->impl->gather_device(d_syms, stride_syms, reinterpret_cast<const PlSyncFrame*>(d_frames), n_streams, wanted_plsc, d_slots, max_slots,
                                             d_offsets, d_slot_record, (hipStream_t)stream));
    API_CATCH
}

} // extern "C"
