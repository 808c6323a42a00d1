// c_api_rotator.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the frequency-correcting rotator.
#include "c_api_common.h"
#include "rotator_hip.h"

using namespace dvbs2;

/* ------------------------------------------------------------------ rotator */
struct dvbs2_rotator {
    RotatorHip* impl = nullptr;
    HostStage stage; enum { BUF, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots"); // grown on demand
    int device = 0;
};

extern "C" {

int dvbs2_rotator_create(dvbs2_rotator_t** h, double phase_inc, int device)
{
    API_TRY
    if (int rc = null_out(h)) return rc;
    if (!(phase_inc == phase_inc) || phase_inc - phase_inc != 0.0) return fail(DVBS2_EINVAL, "phase_inc must be finite");
    return make_handle(h, device, [&] { return new (std::nothrow) RotatorHip(phase_inc, device); });
    API_CATCH
}

void dvbs2_rotator_destroy(dvbs2_rotator_t* h) { destroy_handle(h); }

int dvbs2_rotator_reset(dvbs2_rotator_t* h)
{
    NEED_HANDLE(h);
    h->impl->reset();
    return DVBS2_OK;
}

int dvbs2_rotator_set_phase_inc(dvbs2_rotator_t* h, double phase_inc)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->set_phase_inc(phase_inc));
    API_CATCH
}

int dvbs2_rotator_schedule(dvbs2_rotator_t* h, int64_t offset, double phase_inc)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->schedule(offset, phase_inc));
    API_CATCH
}

int dvbs2_rotator_seek(dvbs2_rotator_t* h, int64_t n_syms)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->seek(n_syms));
    API_CATCH
}

int dvbs2_rotator_position(const dvbs2_rotator_t* h, int64_t* n_syms, int* queued)
{
    NEED_HANDLE(h);
    if (n_syms) *n_syms = h->impl->position();
    if (queued) *queued = h->impl->queued();
    return DVBS2_OK;
}

int dvbs2_rotator_rotate_device(dvbs2_rotator_t* h, const float* d_in, int n_syms, float* d_out, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || (n_syms && (!d_in || !d_out))) return fail(DVBS2_EINVAL, "bad argument");
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) return fail(DVBS2_EINVAL, "symbol buffers must be 8-byte aligned");
    return impl_rc(h, h->impl->rotate_device(d_in, n_syms, d_out, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_rotator_measure(int device, int n_syms, int regions, double* rotate_ms, double* copy_ms)
{
    API_TRY
    if (!rotate_ms || !copy_ms) return fail(DVBS2_EINVAL, "bad argument");
    if (int rc = check_device(device)) return rc;
    std::string err;
    if (int rc = rotator_measure(device, n_syms, regions, rotate_ms, copy_ms, &err)) return fail(rc, err);
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_rotator_rotate(dvbs2_rotator_t* h, const float* in, int n_syms, float* out)
{
    API_TRY
    NEED_HANDLE(h);
    if (n_syms < 0 || (n_syms && (!in || !out))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_syms == 0) return DVBS2_OK;
    HostStage& s = h->stage;
    HostEntry entry(s, h->device);
    if (entry.rc) return entry.rc;
    const size_t bytes = (size_t)n_syms * 8;
    if (int rc = s.ensure(h->BUF, bytes)) return rc;
    float* d_buf = s.at<float>(h->BUF);
    HCHK(hipMemcpyAsync(d_buf, in, bytes, hipMemcpyHostToDevice, s.stream));
    if (int rc = impl_rc(h, h->impl->rotate_device(d_buf, n_syms, d_buf, s.stream))) return rc;
    HCHK(hipMemcpyAsync(out, d_buf, bytes, hipMemcpyDeviceToHost, s.stream));
    return s.sync();
    API_CATCH
}

} // extern "C"
