// c_api_rotator_rows.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the rotator for rows of streams from state in device memory and
// its frequency-control step. No handle type: every entry checks its arguments first, and the device entries look for a device after that.
#include "c_api_common.h"
#include "rotator_rows_hip.h"
#include "rotator_turns.h"

using namespace dvbs2;

static_assert(sizeof(dvbs2_rotator_state_t) == 32 && sizeof(RotatorState) == 32, "the record is 32 bytes");
static_assert(offsetof(dvbs2_rotator_state_t, phase) == offsetof(RotatorState, phase) && offsetof(dvbs2_rotator_state_t, inc) == offsetof(RotatorState, inc) &&
              offsetof(dvbs2_rotator_state_t, index) == offsetof(RotatorState, index) && offsetof(dvbs2_rotator_state_t, reserved) == offsetof(RotatorState, reserved),
              "the header's record is the kernels'");

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

int check_n_streams(int n_streams)
{
    if (n_streams < 1 || n_streams > kRotRowsMaxStreams) return fail(DVBS2_EINVAL, "n_streams out of range (1..65535)");
    return DVBS2_OK;
}

int check_state(const void* d_state)
{
    if (!d_state) return fail(DVBS2_EINVAL, "state is null");
    if ((uintptr_t)d_state & 15) return fail(DVBS2_EINVAL, "state must be 16-byte aligned");
    return DVBS2_OK;
}

// turns (2^-64 units) as radians in (-pi, pi]
double turns_to_radians(uint64_t t)
{
    const long double two_pi = 6.283185307179586476925286766559005768L; // rotator_turns.h's
    const long double signed_turns = t <= (1ull << 63) ? (long double)t : -(long double)(0 - t);
    return (double)(ldexpl(signed_turns, -64) * two_pi);
}

int launched(hipError_t e, const char* what)
{
    if (e != hipSuccess) return fail(DVBS2_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return DVBS2_OK;
}

} // namespace

extern "C" {

int dvbs2_rotator_state_init(const double* phase_inc, int n_streams, dvbs2_rotator_state_t* state)
{
    API_TRY
    if (int rc = check_n_streams(n_streams)) return rc;
    if (!phase_inc) return fail(DVBS2_EINVAL, "phase_inc is null");
    if (!state) return fail(DVBS2_EINVAL, "state is null");
    for (int s = 0; s < n_streams; s++)
        if (!is_finite(phase_inc[s])) return fail(DVBS2_EINVAL, "phase_inc[" + std::to_string(s) + "] must be finite");
    for (int s = 0; s < n_streams; s++) state[s] = dvbs2_rotator_state_t{ 0, rotator_inc_turns(phase_inc[s]), 0, 0 };
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_state_read(const dvbs2_rotator_state_t* state, int n_streams, double* phase_inc, double* phase_at_index)
{
    API_TRY
    if (int rc = check_n_streams(n_streams)) return rc;
    if (!state) return fail(DVBS2_EINVAL, "state is null");
    for (int s = 0; s < n_streams; s++) {
        if (phase_inc) phase_inc[s] = turns_to_radians(state[s].inc);
        if (phase_at_index) phase_at_index[s] = turns_to_radians(state[s].phase);
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_adjust_turns(float estimate, double scale, int64_t* delta, int* applies)
{
    API_TRY
    if (!delta) return fail(DVBS2_EINVAL, "delta is null");
    if (!applies) return fail(DVBS2_EINVAL, "applies is null");
    *applies = rotator_adjust_turns(estimate, scale, delta) ? 1 : 0;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_rows_check(int64_t in_stride, int64_t out_stride, int n_samples, int n_streams, int64_t base_index)
{
    API_TRY
    const std::string bad = rotator_rows_check(in_stride, out_stride, n_samples, n_streams, base_index);
    if (!bad.empty()) return fail(DVBS2_EINVAL, bad);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_rows_device(const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int n_samples, int n_streams,
                              int64_t base_index, const dvbs2_rotator_state_t* d_state, int device, void* stream)
{
    API_TRY
    if (int rc = dvbs2_rotator_rows_check(in_stride, out_stride, n_samples, n_streams, base_index)) return rc;
    if (n_samples == 0) return DVBS2_OK;
    if (int rc = check_in_out(d_in, d_out)) return rc;
    if (int rc = check_aligned8(d_in, d_out)) return rc;
    if (n_streams > 1 && d_in == d_out && in_stride != out_stride) return fail(DVBS2_EINVAL, "in place needs equal strides");
    if (int rc = check_state(d_state)) return rc;
    if (int rc = check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    return launched(rotator_rows_launch(d_in, in_stride, d_out, out_stride, n_samples, n_streams, base_index,
                                        reinterpret_cast<const RotatorState*>(d_state), (hipStream_t)stream), "rotator rows kernel launch");
    API_CATCH
}

int dvbs2_rotator_retune_device(dvbs2_rotator_state_t* d_state, int stream_index, int64_t at_index, double phase_inc, int device, void* stream)
{
    API_TRY
    if (int rc = check_state(d_state)) return rc;
    if (stream_index < 0 || stream_index >= kRotRowsMaxStreams) return fail(DVBS2_EINVAL, "stream_index out of range (0..65534)");
    if (at_index < 0) return fail(DVBS2_EINVAL, "at_index is negative");
    if (!is_finite(phase_inc)) return fail(DVBS2_EINVAL, "phase_inc must be finite");
    if (int rc = check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    return launched(rotator_retune_launch(reinterpret_cast<RotatorState*>(d_state), stream_index, at_index, rotator_inc_turns(phase_inc),
                                          (hipStream_t)stream), "rotator retune kernel launch");
    API_CATCH
}

int dvbs2_rotator_control_device(const int32_t* d_offsets, int n_streams, int max_slots, const float* d_coarse_foffset,
                                 const int32_t* d_coarse_corrected, const int32_t* d_new_est, const float* d_fine_foffset,
                                 const int32_t* d_fine_valid, double coarse_scale, double fine_scale, int64_t at_index,
                                 dvbs2_rotator_state_t* d_state, int32_t* d_applied, int64_t* d_delta, int device, void* stream)
{
    API_TRY
    if (int rc = check_n_streams(n_streams)) return rc;
    if (max_slots < 0) return fail(DVBS2_EINVAL, "max_slots is negative");
    if (!d_offsets) return fail(DVBS2_EINVAL, "offsets is null");
    if (!d_coarse_foffset) return fail(DVBS2_EINVAL, "coarse_foffset is null");
    if (!d_coarse_corrected) return fail(DVBS2_EINVAL, "coarse_corrected is null");
    if (!d_new_est) return fail(DVBS2_EINVAL, "new_est is null");
    if (!d_fine_foffset != !d_fine_valid) return fail(DVBS2_EINVAL, "fine_foffset and fine_valid go together");
    if (((uintptr_t)d_offsets | (uintptr_t)d_coarse_foffset | (uintptr_t)d_coarse_corrected | (uintptr_t)d_new_est | (uintptr_t)d_fine_foffset |
         (uintptr_t)d_fine_valid | (uintptr_t)d_applied) & 3)
        return fail(DVBS2_EINVAL, "the per-slot and per-stream arrays must be 4-byte aligned");
    if ((uintptr_t)d_delta & 7) return fail(DVBS2_EINVAL, "delta must be 8-byte aligned");
    if (!is_finite(coarse_scale)) return fail(DVBS2_EINVAL, "coarse_scale must be finite");
    if (!is_finite(fine_scale)) return fail(DVBS2_EINVAL, "fine_scale must be finite");
    if (at_index < 0) return fail(DVBS2_EINVAL, "at_index is negative");
    if (int rc = check_state(d_state)) return rc;
    if (int rc = check_device(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    return launched(rotator_control_launch(d_offsets, n_streams, max_slots, d_coarse_foffset, d_coarse_corrected, d_new_est, d_fine_foffset,
                                           d_fine_valid, coarse_scale, fine_scale, at_index, reinterpret_cast<RotatorState*>(d_state), d_applied,
                                           d_delta, (hipStream_t)stream), "rotator control kernel launch");
    API_CATCH
}

} // extern "C"
