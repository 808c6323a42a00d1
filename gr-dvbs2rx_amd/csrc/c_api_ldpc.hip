// c_api_ldpc.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the LDPC decoder handle.
#include <cstdlib>
#include "c_api_fec.h"
#include "fec_tables.h"
#include "host_plan.h"

using namespace dvbs2;

static int ldpc_make(dvbs2_ldpc_t** h, const LdpcTableDesc* t, int message_bits, int G, int max_frames, int device)
{
    if (int rc = null_out(h)) return rc;
    if (!t) return fail(DVBS2_EINVAL, "unknown LDPC table");
    if (int rc = make_handle(h, device, [&] { return new (std::nothrow) LdpcDecoderHip(t, message_bits, G, max_frames, device); })) return rc;
    if (const char* e = getenv("DVBS2_HOST_PLAN")) (*h)->host_plan = e;
    if (const char* e = getenv("DVBS2_HOST_CHUNK")) (*h)->host_chunk = std::max(2, atoi(e));
    if (const char* e = getenv("DVBS2_HOST_COPY_STREAM")) (*h)->host_copy_stream = atoi(e) != 0 ? 1 : 0;
    return DVBS2_OK;
}

extern "C" {

int dvbs2_ldpc_create(dvbs2_ldpc_t** h, int standard, int framesize, int rate, int group_size, int max_frames, int device)
{
    API_TRY
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi) || !fi.table) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    return ldpc_make(h, fi.table, (int)fi.ldpc_k, group_size, max_frames, device);
    API_CATCH
}

int dvbs2_ldpc_create_table(dvbs2_ldpc_t** h, const char* table, int message_bits, int group_size, int max_frames, int device)
{
    API_TRY
    return ldpc_make(h, find_ldpc_table(table), message_bits, group_size, max_frames, device);
    API_CATCH
}

void dvbs2_ldpc_destroy(dvbs2_ldpc_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    h->stage.release();
    host_pipe_destroy(h->pipe);
    delete h->impl;
    delete h;
}

int dvbs2_ldpc_params(const dvbs2_ldpc_t* h, int* n, int* table_k, int* message_bits, int* q, int* group_size)
{
    NEED_HANDLE(h);
    if (n) *n = h->impl->N(); if (table_k) *table_k = h->impl->K();
    if (message_bits) *message_bits = h->impl->out_bits_message();
    if (q) *q = h->impl->q(); if (group_size) *group_size = h->impl->group_size();
    return DVBS2_OK;
}

static int ldpc_check_args(dvbs2_ldpc_t* h, const void* in, int n_frames, int max_trials, int out_mode, const void* bits,
                           const void* d_llr_out = nullptr, bool device_pointers = false)
{
    NEED_HANDLE(h);
    if (n_frames < 0 || max_trials <= 0 || (n_frames && (!in || !bits))) return fail(DVBS2_EINVAL, "bad argument");
    // the kernels move LLRs with 8-byte loads and stores (include/dvbs2_fec_hip.h): a misaligned device pointer would be a GPU memory fault
    if (device_pointers && ((((uintptr_t)in) | ((uintptr_t)d_llr_out)) & 7u)) return fail(DVBS2_EINVAL, "d_llr_in / d_llr_out must be 8-byte aligned");
    if (out_mode != DVBS2_OM_CODEWORD && out_mode != DVBS2_OM_MESSAGE) return fail(DVBS2_EINVAL, "bad out_mode");
    if (n_frames > h->impl->max_frames()) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    return DVBS2_OK;
}

int dvbs2_ldpc_decode_device(dvbs2_ldpc_t* h, const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode,
                             uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret, void* stream)
{
    API_TRY
    if (int rc = ldpc_check_args(h, d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, true)) return rc;
    return impl_rc(h, h->impl->decode_device(d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, d_ret, (hipStream_t)stream));
    API_CATCH
}

int dvbs2_ldpc_enqueue_device(dvbs2_ldpc_t* h, const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode,
                              uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret, void* stream)
{
    API_TRY
    if (int rc = ldpc_check_args(h, d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, true)) return rc;
    return impl_rc(h, h->impl->enqueue(d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, d_ret, (hipStream_t)stream, 0, 0));
    API_CATCH
}

int dvbs2_ldpc_finish(dvbs2_ldpc_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    return impl_rc(h, h->impl->finish(0) < 0);
    API_CATCH
}

int dvbs2_ldpc_decode(dvbs2_ldpc_t* h, const int8_t* llr_in, int n_frames, int max_trials, int out_mode,
                      uint8_t* bits_out, int8_t* llr_out, int32_t* ret)
{
    API_TRY
    if (int rc = ldpc_check_args(h, llr_in, n_frames, max_trials, out_mode, bits_out)) return rc;
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    LdpcDecoderHip* dec = h->impl;
    const size_t N = dec->N(), mf = dec->max_frames();
    const int G = dec->group_size();
    const size_t ret_bytes = ((mf + G - 1) / G + kSlots) * 4;
    if (int rc = host_pipe_init(h->pipe)) return rc;
    HostStage& s = h->stage;
    if (s.ensure(h->IN, mf * N) || s.ensure(h->BITS, mf * (N / 8)) || s.ensure(h->LLR, mf * N) || s.ensure(h->RET, ret_bytes)) return DVBS2_EDEVICE;
    int8_t* d_in = s.at<int8_t>(h->IN); uint8_t* d_bits = s.at<uint8_t>(h->BITS);
    int8_t* d_llr = s.at<int8_t>(h->LLR); int32_t* d_ret = s.at<int32_t>(h->RET);
    const size_t out_bytes = (out_mode ? dec->out_bits_message() : (int)N) / 8;
    HostCall call;
    if (int rc = host_add_output(h->pipe, call, n_frames, d_bits, bits_out, out_bytes, 1, mf * (N / 8))) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, d_llr, llr_out, N, 1, mf * N)) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, d_ret, ret, 4, G, ret_bytes)) return rc;
    const bool in_locked = host_range_page_locked(llr_in, (size_t)n_frames * N);
    call.plan = host_chunk_plan(n_frames, G, in_locked, false, h->host_chunk, h->host_plan);
    call.use_copy_stream = h->host_copy_stream >= 0 ? h->host_copy_stream != 0 : in_locked; // (DVBS2_HOST_COPY_STREAM: experiments)
    call.copy_in = [&](int, int f0, int nf, hipStream_t cs) -> int {
        HCHK(hipMemcpyAsync(d_in + (size_t)f0 * N, llr_in + (size_t)f0 * N, (size_t)nf * N, hipMemcpyHostToDevice, cs));
        return DVBS2_OK;
    };
    call.enqueue = [&](int c, int f0, int nf, hipStream_t st) -> int {
        return impl_rc(h, dec->enqueue(d_in + (size_t)f0 * N, nf, max_trials, out_mode, d_bits + (size_t)f0 * out_bytes,
                                       llr_out ? d_llr + (size_t)f0 * N : nullptr, d_ret + f0 / G, st, c % kSlots, f0));
    };
    return host_pipe_run(h->pipe, dec, call); // (nothing after the LDPC: outputs that extra rounds rewrote are only fetched again)
    API_CATCH
}

const char* dvbs2_ldpc_kernel_name(const dvbs2_ldpc_t* h) { return h ? h->impl->kernel_name() : nullptr; }
int dvbs2_ldpc_fallback_rounds(const dvbs2_ldpc_t* h) { return h ? h->impl->fallback_rounds() : -1; }

int dvbs2_ldpc_profile(dvbs2_ldpc_t* h, int enable, double* total_ms, int* launches)
{
    NEED_HANDLE(h);
    if (total_ms) *total_ms = h->impl->profile_ms();
    if (launches) *launches = h->impl->profile_launches();
    h->impl->set_profiling(enable != 0);
    if (enable) h->impl->reset_profile();
    return DVBS2_OK;
}

} // extern "C"
