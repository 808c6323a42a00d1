// c_api_bbdeheader_rows.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the BBFRAME de-header for rows of streams from state in
// device memory. No handle type: every entry checks its arguments first, and the device entry looks for a device after that.
#include "c_api_common.h"
#include "bbdeheader_rows_hip.h"

using namespace dvbs2;

static_assert(sizeof(dvbs2_bbdeheader_state_t) == 256 && sizeof(BbdhRow) == 256, "the record is 256 bytes");
static_assert(offsetof(dvbs2_bbdeheader_state_t, synched) == offsetof(BbdhRow, synched) && offsetof(dvbs2_bbdeheader_state_t, partial_ts_bytes) == offsetof(BbdhRow, partial) &&
              offsetof(dvbs2_bbdeheader_state_t, packets) == offsetof(BbdhRow, packets) && offsetof(dvbs2_bbdeheader_state_t, errors) == offsetof(BbdhRow, errors) &&
              offsetof(dvbs2_bbdeheader_state_t, bbframes) == offsetof(BbdhRow, bbframes) && offsetof(dvbs2_bbdeheader_state_t, dropped) == offsetof(BbdhRow, dropped) &&
              offsetof(dvbs2_bbdeheader_state_t, gaps) == offsetof(BbdhRow, gaps) && offsetof(dvbs2_bbdeheader_state_t, overruns) == offsetof(BbdhRow, overruns) &&
              offsetof(dvbs2_bbdeheader_state_t, last_packets) == offsetof(BbdhRow, last_packets) && offsetof(dvbs2_bbdeheader_state_t, reserved) == offsetof(BbdhRow, reserved) &&
              offsetof(dvbs2_bbdeheader_state_t, partial_pkt) == offsetof(BbdhRow, partial_pkt) && sizeof(((dvbs2_bbdeheader_state_t*)0)->partial_pkt) == kTsLen,
              "the header's record is the kernels'");

extern "C" {

int dvbs2_bbdeheader_rows_check(int kbch_bits, int n_streams, int max_frames)
{
    API_TRY
    const std::string bad = bbdeheader_rows_check(kbch_bits, n_streams, max_frames);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_rows_geometry(int kbch_bits, int n_streams, int max_frames, int* kbch_bytes, int* max_out_bytes_per_frame, int64_t* work_bytes,
                                   int64_t* out_bytes)
{
    API_TRY
    if (int rc = dvbs2_bbdeheader_rows_check(kbch_bits, n_streams, max_frames)) return rc;
    const BbdhRowsGeometry g = bbdeheader_rows_geometry(kbch_bits, n_streams, max_frames);
    if (kbch_bytes) *kbch_bytes = g.kbch_bytes;
    if (max_out_bytes_per_frame) *max_out_bytes_per_frame = g.max_out_bytes_per_frame;
    if (work_bytes) *work_bytes = g.work_bytes;
    if (out_bytes) *out_bytes = g.out_bytes;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_state_counters(const dvbs2_bbdeheader_state_t* state, int n_streams, dvbs2_bbdeheader_counters_t* out)
{
    API_TRY
    if (n_streams < 1 || n_streams > kBbdhRowsMaxStreams) return fail(DVBS2_EINVAL, "n_streams out of range (1..1024)");
    if (!state) return fail(DVBS2_EINVAL, "state is null");
    if (!out) return fail(DVBS2_EINVAL, "out is null");
    for (int s = 0; s < n_streams; s++) {
        const dvbs2_bbdeheader_state_t& r = state[s];
        dvbs2_bbdeheader_counters_t& o = out[s];
        o.packets = r.packets; o.errors = r.errors; o.bbframes = r.bbframes; o.dropped = r.dropped; o.gaps = r.gaps; o.overruns = r.overruns;
        o.synched = r.synched; o.partial_ts_bytes = r.partial_ts_bytes;
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_bbdeheader_rows_device(const uint8_t* d_bbframes, int kbch_bits, const int32_t* d_offsets, int n_streams, int max_frames,
                                 dvbs2_bbdeheader_state_t* d_state, void* d_work, int64_t work_bytes, uint8_t* d_ts_out, int64_t out_bytes,
                                 int32_t* d_pkt_offsets, int device, void* stream)
{
    API_TRY
    if (int rc = dvbs2_bbdeheader_rows_check(kbch_bits, n_streams, max_frames)) return rc;
    if (!d_bbframes) return fail(DVBS2_EINVAL, "bbframes is null");
    if (!d_offsets) return fail(DVBS2_EINVAL, "offsets is null");
    if (!d_state) return fail(DVBS2_EINVAL, "state is null");
    if (!d_work) return fail(DVBS2_EINVAL, "work is null");
    if (!d_ts_out) return fail(DVBS2_EINVAL, "ts_out is null");
    if (!d_pkt_offsets) return fail(DVBS2_EINVAL, "pkt_offsets is null");
    if (((uintptr_t)d_offsets | (uintptr_t)d_pkt_offsets) & 3) return fail(DVBS2_EINVAL, "offsets and pkt_offsets must be 4-byte aligned");
    if ((uintptr_t)d_state & 15) return fail(DVBS2_EINVAL, "state must be 16-byte aligned");
    if ((uintptr_t)d_work & 15) return fail(DVBS2_EINVAL, "work must be 16-byte aligned");
    const BbdhRowsGeometry g = bbdeheader_rows_geometry(kbch_bits, n_streams, max_frames);
    if (work_bytes < g.work_bytes) return fail(DVBS2_ESIZE, "work_bytes is below the geometry's " + std::to_string(g.work_bytes));
    if (out_bytes < g.out_bytes) return fail(DVBS2_ESIZE, "out_bytes is below the geometry's " + std::to_string(g.out_bytes));
    if (int rc = check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    const hipError_t e = bbdeheader_rows_launch(d_bbframes, kbch_bits, d_offsets, n_streams, max_frames, reinterpret_cast<BbdhRow*>(d_state), d_work,
                                                d_ts_out, out_bytes, d_pkt_offsets, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DVBS2_EDEVICE, std::string("bbdeheader rows kernel launch: ") + hipGetErrorString(e));
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
