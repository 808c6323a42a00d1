// c_api_chain.hip -- extern "C" boundary (include/dvbs2_fec_hip.h): the fused demapper -> LDPC -> BCH chain.
#include "c_api_fec.h"
#include "host_plan.h"

using namespace dvbs2;

struct dvbs2_chain {
    dvbs2_demap_t* dm = nullptr; // absent for an LLR-domain chain (dvbs2_chain_create_llr)
    dvbs2_ldpc_t* ldpc = nullptr; dvbs2_bch_t* bch = nullptr;
    int8_t* d_llr = nullptr; uint8_t* d_bits = nullptr; int32_t* d_corr = nullptr;
    int device = 0, max_frames = 0, n_llr = 0, ldpc_bytes = 0, msg_bytes = 0;
    // the call between enqueue and finish
    bool pending = false; int n_frames = 0; uint8_t* d_msg = nullptr; int32_t* d_bch_corr = nullptr; void* stream = nullptr;
    // host-pointer entries (dvbs2_chain_decode / dvbs2_chain_decode_llr): device copies of the caller's buffers in `stage` (its stream stays
    // unused), pinned landing buffers for the outputs of a pageable caller and the streams in `pipe` (as dvbs2_ldpc_decode)
    HostStage stage; enum { SYMS, LLR, N0, MSG, RET, CORR, N_SLOTS }; static_assert(N_SLOTS <= HostStage::kBufs, "too many staging slots");
    HostPipe pipe;
};

// table != nullptr: the demapper of a caller's table (dvbs2_demap_create_table), `constellation` unused
struct ChainTable { int n_mod; const float* points_re_im; const uint8_t* column; };
static int chain_make(dvbs2_chain_t** h, int standard, int framesize, int rate, int constellation, bool with_demap,
                      int group_size, int max_frames, int device, const ChainTable* table = nullptr)
{
    if (int rc = null_out(h)) return rc;
    dvbs2_chain* o = new (std::nothrow) dvbs2_chain();
    if (!o) return fail(DVBS2_EDEVICE, "out of memory");
    o->device = device; o->max_frames = max_frames;
    int rc = DVBS2_OK;
    if (table) rc = dvbs2_demap_create_table(&o->dm, framesize, table->n_mod, table->points_re_im, table->column, max_frames, device);
    else if (with_demap) rc = dvbs2_demap_create(&o->dm, framesize, rate, constellation, max_frames, device);
    if (rc == DVBS2_OK) rc = dvbs2_ldpc_create(&o->ldpc, standard, framesize, rate, group_size, max_frames, device);
    if (rc == DVBS2_OK) rc = dvbs2_bch_create(&o->bch, standard, framesize, rate, max_frames, device);
    if (rc != DVBS2_OK) { std::string keep = g_api_error; dvbs2_chain_destroy(o); return fail(rc, keep); }
    o->n_llr = o->ldpc->impl->N();
    o->ldpc_bytes = o->ldpc->impl->out_bits_message() / 8;
    o->msg_bytes = o->bch->impl->code().k / 8;
    if ((o->dm && o->dm->impl->n_llr() != o->n_llr) || o->ldpc_bytes != o->bch->impl->code().n / 8) { dvbs2_chain_destroy(o); return fail(DVBS2_EINVAL, "inconsistent chain sizes"); }
    DeviceGuard guard(device);
    hipError_t e = guard.ok ? hipSuccess : hipErrorInvalidDevice;
    if (e == hipSuccess && o->dm) e = hipMalloc(&o->d_llr, (size_t)max_frames * o->n_llr);
    if (e == hipSuccess) e = hipMalloc(&o->d_bits, (size_t)max_frames * o->ldpc_bytes);
    if (e == hipSuccess) e = hipMalloc(&o->d_corr, (size_t)max_frames * 4);
    if (e != hipSuccess) { dvbs2_chain_destroy(o); return fail(DVBS2_EDEVICE, hipGetErrorString(e)); }
    *h = o;
    return DVBS2_OK;
}

// LDPC (already enqueued) -> BCH on the same stream; the LDPC output never leaves HBM
// BCH straight from the LDPC decoder's state (hard decision + packing of ldpc_decoder_bb fused into the BCH kernel's load: no
// finalize launch, no packed-bit buffer in between)
static int chain_bch_range(dvbs2_chain_t* h, int frame_base, int n_frames, uint8_t* d_msg, int32_t* d_corr, hipStream_t stream)
{
    const int N = h->ldpc->impl->N();
    return impl_rc(h->bch, h->bch->impl->decode_device(nullptr, n_frames, d_msg, d_corr, stream, h->ldpc->impl->state() + (size_t)frame_base * N, N, frame_base));
}
static int chain_bch(dvbs2_chain_t* h) { return chain_bch_range(h, 0, h->n_frames, h->d_msg, h->d_bch_corr, (hipStream_t)h->stream); }

// LDPC -> BCH on one stream; dm != nullptr: the LDPC sweep kernel demaps the symbols while it loads them
static int chain_enqueue_tail(dvbs2_chain_t* h, const int8_t* d_llr, const DemapFused* dm, int n_frames, int max_trials, uint8_t* d_msg,
                              int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    if (int rc = impl_rc(h->ldpc, h->ldpc->impl->enqueue(d_llr, n_frames, max_trials, DVBS2_OM_MESSAGE, nullptr, nullptr, d_ldpc_ret, (hipStream_t)stream, 0, 0, dm))) return rc;
    h->pending = true; h->n_frames = n_frames; h->d_msg = d_msg; h->d_bch_corr = d_bch_corr ? d_bch_corr : h->d_corr; h->stream = stream;
    const int rc = chain_bch(h);
    if (rc != DVBS2_OK) { h->ldpc->impl->abort_all(); h->pending = false; } // nothing stays in flight or busy after a failed call
    return rc;
}

extern "C" {

int dvbs2_chain_set_descramble(dvbs2_chain_t* h, int enable)
{
    NEED_HANDLE(h);
    return dvbs2_bch_set_descramble(h->bch, enable);
}

void dvbs2_chain_destroy(dvbs2_chain_t* h)
{
    if (!h) return;
    DeviceGuard guard(h->device);
    dvbs2_demap_destroy(h->dm); dvbs2_ldpc_destroy(h->ldpc); dvbs2_bch_destroy(h->bch);
    (void)hipFree(h->d_llr); (void)hipFree(h->d_bits); (void)hipFree(h->d_corr);
    h->stage.release();
    host_pipe_destroy(h->pipe);
    delete h;
}

int dvbs2_chain_create(dvbs2_chain_t** h, int standard, int framesize, int rate, int constellation, int group_size, int max_frames, int device)
{
    API_TRY
    return chain_make(h, standard, framesize, rate, constellation, true, group_size, max_frames, device);
    API_CATCH
}

int dvbs2_chain_create_table(dvbs2_chain_t** h, int standard, int framesize, int rate, int n_mod, const float* points_re_im,
                             const uint8_t* column, int group_size, int max_frames, int device)
{
    API_TRY
    const ChainTable table = { n_mod, points_re_im, column };
    return chain_make(h, standard, framesize, rate, 0, true, group_size, max_frames, device, &table);
    API_CATCH
}

int dvbs2_chain_create_llr(dvbs2_chain_t** h, int standard, int framesize, int rate, int group_size, int max_frames, int device)
{
    API_TRY
    return chain_make(h, standard, framesize, rate, 0, false, group_size, max_frames, device);
    API_CATCH
}

int dvbs2_chain_params(const dvbs2_chain_t* h, int* n_syms, int* msg_bytes)
{
    NEED_HANDLE(h);
    if (n_syms) *n_syms = h->dm ? h->dm->impl->n_syms() : 0;
    if (msg_bytes) *msg_bytes = h->msg_bytes;
    return DVBS2_OK;
}

int dvbs2_chain_llr_params(const dvbs2_chain_t* h, int* n_llr, int* msg_bytes, int* group_size)
{
    NEED_HANDLE(h);
    if (n_llr) *n_llr = h->n_llr;
    if (msg_bytes) *msg_bytes = h->msg_bytes;
    if (group_size) *group_size = h->ldpc->impl->group_size();
    return DVBS2_OK;
}

int dvbs2_chain_enqueue_device(dvbs2_chain_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count,
                               int max_trials, uint8_t* d_msg, int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (!h->dm) return fail(DVBS2_EINVAL, "this chain starts at LLRs: use dvbs2_chain_enqueue_llr_device");
    if (h->pending) return fail(DVBS2_EINVAL, "previous call not finished");
    if (n_frames > h->max_frames) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && !d_msg)) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames == 0) return DVBS2_OK;
    if (!d_syms || !d_n0 || (n0_count != 1 && n0_count != n_frames)) return fail(DVBS2_EINVAL, "bad argument");
    if (h->ldpc->impl->fused_demap_supported() && h->dm->impl->fusable()) { // symbols -> LDS inside the LDPC sweep kernel: no demapper launch, no LLR buffer
        const DemapFused dm = h->dm->impl->fused(d_syms, d_n0, n0_count);
        return chain_enqueue_tail(h, nullptr, &dm, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    }
    int rc = dvbs2_demap_soft_device(h->dm, d_syms, n_frames, d_n0, n0_count, h->d_llr, stream);
    if (rc == DVBS2_OK) rc = chain_enqueue_tail(h, h->d_llr, nullptr, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    return rc;
    API_CATCH
}

int dvbs2_chain_enqueue_llr_device(dvbs2_chain_t* h, const int8_t* d_llr, int n_frames, int max_trials, uint8_t* d_msg,
                                   int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    API_TRY
    NEED_HANDLE(h);
    if (h->pending) return fail(DVBS2_EINVAL, "previous call not finished");
    if (n_frames > h->max_frames) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && (!d_llr || !d_msg))) return fail(DVBS2_EINVAL, "bad argument");
    if (((uintptr_t)d_llr) & 7u) return fail(DVBS2_EINVAL, "d_llr must be 8-byte aligned"); // (8-byte loads: include/dvbs2_fec_hip.h)
    if (n_frames == 0) return DVBS2_OK;
    return chain_enqueue_tail(h, d_llr, nullptr, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    API_CATCH
}

int dvbs2_chain_ldpc_profile(dvbs2_chain_t* h, int enable, double* total_ms, int* launches)
{
    NEED_HANDLE(h);
    return dvbs2_ldpc_profile(h->ldpc, enable, total_ms, launches);
}

const char* dvbs2_chain_ldpc_kernel_name(const dvbs2_chain_t* h) { return h ? h->ldpc->impl->kernel_name() : nullptr; }
int dvbs2_chain_ldpc_fallback_rounds(const dvbs2_chain_t* h) { return h ? h->ldpc->impl->fallback_rounds() : -1; }

int dvbs2_chain_finish(dvbs2_chain_t* h)
{
    API_TRY
    NEED_HANDLE(h);
    if (!h->pending) return DVBS2_OK;
    h->pending = false;
    const int r = h->ldpc->impl->finish(0); // waits for the stream: demapper, LDPC and BCH of this call are done
    if (r < 0) return impl_rc(h->ldpc, true);
    if (r > 0) { // the LDPC needed rounds beyond the enqueued ones and rewrote its output: run the BCH stage again
        int rc = chain_bch(h);
        if (rc != DVBS2_OK) return rc;
        HCHK(hipStreamSynchronize((hipStream_t)h->stream));
    }
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_chain_decode_device(dvbs2_chain_t* h, const float* d_syms, int n_frames, const float* d_n0, int n0_count,
                              int max_trials, uint8_t* d_msg, int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    int rc = dvbs2_chain_enqueue_device(h, d_syms, n_frames, d_n0, n0_count, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    if (rc != DVBS2_OK) { if (h) h->pending = false; return rc; }
    return dvbs2_chain_finish(h);
}

int dvbs2_chain_decode_llr_device(dvbs2_chain_t* h, const int8_t* d_llr, int n_frames, int max_trials, uint8_t* d_msg,
                                  int32_t* d_ldpc_ret, int32_t* d_bch_corr, void* stream)
{
    int rc = dvbs2_chain_enqueue_llr_device(h, d_llr, n_frames, max_trials, d_msg, d_ldpc_ret, d_bch_corr, stream);
    if (rc != DVBS2_OK) { if (h) h->pending = false; return rc; }
    return dvbs2_chain_finish(h);
}

} // extern "C"

// Host-pointer form of the fused chain (SURVEY 8(b) "dvbs2_fec_chain_decode(syms -> msg bytes)"): what the three blocks do with the
// item buffers GNU Radio hands them (lib/xfecframe_demapper_cb_impl.cc:101-186 -> lib/ldpc_decoder_bb_impl.cc:394-455 ->
// lib/bch_decoder_bb_impl.cc:84-117), as ONE call. The call is cut into chunks of whole LDPC groups and goes through host_pipe_run like
// dvbs2_ldpc_decode: chunk c runs on stream c mod kSlots in its own range of the LDPC state / message buffers and of the BCH syndrome words, its input
// copy (through one copy stream when the caller's buffer is page-locked) runs under the kernels of chunk c - 1 and its results go
// back while chunk c + 1 decodes. An 8PSK normal frame is 172.8 KB of symbols in and ~6 KB out: at the ~57 GB/s of the host link the
// chain is LINK-bound near 320 k frames/s -- below what the kernels do at a receiver's operating point (bench.py config3_host).
// in_syms: XFECFRAME symbols (a demapping chain) or null; in_llr: int8 LLRs (either kind of chain) or null.
static int chain_decode_host(dvbs2_chain_t* h, const float* in_syms, const int8_t* in_llr, int n_frames, const float* n0, int n0_count,
                             int max_trials, uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr)
{
    NEED_HANDLE(h);
    if (h->pending) return fail(DVBS2_EINVAL, "previous call not finished");
    if (n_frames > h->max_frames) return fail(DVBS2_ESIZE, "n_frames exceeds max_frames");
    if (n_frames < 0 || max_trials <= 0 || (n_frames && (!msg || (!in_syms && !in_llr)))) return fail(DVBS2_EINVAL, "bad argument");
    if (in_syms && !h->dm) return fail(DVBS2_EINVAL, "this chain starts at LLRs: use dvbs2_chain_decode_llr");
    if (in_syms && (!n0 || (n0_count != 1 && n0_count != n_frames))) return fail(DVBS2_EINVAL, "bad argument");
    if (n_frames == 0) return DVBS2_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    LdpcDecoderHip* dec = h->ldpc->impl;
    const size_t N = (size_t)dec->N(), mf = (size_t)h->max_frames, mb = (size_t)h->msg_bytes;
    const size_t ns = h->dm ? (size_t)h->dm->impl->n_syms() : 0;
    const int G = dec->group_size();
    const size_t ret_bytes = ((mf + G - 1) / G + kSlots) * 4;
    if (int rc = host_pipe_init(h->pipe)) return rc;
    const bool fused = in_syms && dec->fused_demap_supported() && h->dm->impl->fusable(); // symbols -> LDS inside the sweep kernel; else demapper launch -> LLR buffer
    HostStage& s = h->stage;
    if (in_syms && (s.ensure(h->SYMS, mf * ns * 8) || s.ensure(h->N0, mf * 4))) return DVBS2_EDEVICE;
    if ((in_llr || !fused) && s.ensure(h->LLR, mf * N)) return DVBS2_EDEVICE;
    if (s.ensure(h->MSG, mf * mb) || s.ensure(h->RET, ret_bytes) || s.ensure(h->CORR, mf * 4)) return DVBS2_EDEVICE;
    float* hd_syms = s.at<float>(h->SYMS); int8_t* hd_llr = s.at<int8_t>(h->LLR); float* hd_n0 = s.at<float>(h->N0);
    uint8_t* hd_msg = s.at<uint8_t>(h->MSG); int32_t* hd_ret = s.at<int32_t>(h->RET); int32_t* hd_corr = s.at<int32_t>(h->CORR);
    HostCall call;
    if (int rc = host_add_output(h->pipe, call, n_frames, hd_msg, msg, mb, 1, mf * mb)) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, hd_ret, ldpc_ret, 4, G, ret_bytes)) return rc;
    if (int rc = host_add_output(h->pipe, call, n_frames, hd_corr, bch_corr, 4, 1, mf * 4)) return rc;
    const void* in_ptr = in_syms ? (const void*)in_syms : (const void*)in_llr;
    const size_t in_frame_bytes = in_syms ? ns * 8 : N;
    const bool in_locked = host_range_page_locked(in_ptr, (size_t)n_frames * in_frame_bytes);
    call.plan = host_chunk_plan(n_frames, G, in_locked, in_syms != nullptr, h->ldpc->host_chunk, "");
    call.use_copy_stream = in_locked;
    call.shared_input = in_syms && n0_count == 1;
    call.copy_in = [&](int c, int f0, int nf, hipStream_t cs) -> int {
        if (in_syms) {
            HCHK(hipMemcpyAsync(hd_syms + (size_t)f0 * ns * 2, in_syms + (size_t)f0 * ns * 2, (size_t)nf * ns * 8, hipMemcpyHostToDevice, cs));
            if (n0_count > 1) HCHK(hipMemcpyAsync(hd_n0 + f0, n0 + f0, (size_t)nf * 4, hipMemcpyHostToDevice, cs));
            else if (c == 0) HCHK(hipMemcpyAsync(hd_n0, n0, 4, hipMemcpyHostToDevice, cs));
        } else
            HCHK(hipMemcpyAsync(hd_llr + (size_t)f0 * N, in_llr + (size_t)f0 * N, (size_t)nf * N, hipMemcpyHostToDevice, cs));
        return DVBS2_OK;
    };
    call.enqueue = [&](int c, int f0, int nf, hipStream_t st) -> int {
        const float* dn0 = n0_count > 1 ? hd_n0 + f0 : hd_n0;
        const float* dsy = in_syms ? hd_syms + (size_t)f0 * ns * 2 : nullptr;
        int erc;
        if (fused) {
            const DemapFused dm = h->dm->impl->fused(dsy, dn0, n0_count > 1 ? nf : 1);
            erc = dec->enqueue(nullptr, nf, max_trials, DVBS2_OM_MESSAGE, nullptr, nullptr, hd_ret + f0 / G, st, c % kSlots, f0, &dm);
        } else {
            if (in_syms && h->dm->impl->soft_device(dsy, nf, dn0, n0_count > 1 ? nf : 1, hd_llr + (size_t)f0 * N, st)) return impl_rc(h->dm, true);
            erc = dec->enqueue(hd_llr + (size_t)f0 * N, nf, max_trials, DVBS2_OM_MESSAGE, nullptr, nullptr, hd_ret + f0 / G, st, c % kSlots, f0, nullptr);
        }
        return impl_rc(h->ldpc, erc != 0);
    };
    call.after_ldpc = [&](int f0, int nf, hipStream_t st) -> int { return chain_bch_range(h, f0, nf, hd_msg + (size_t)f0 * mb, hd_corr + f0, st); };
    return host_pipe_run(h->pipe, dec, call);
}

extern "C" {

int dvbs2_chain_decode(dvbs2_chain_t* h, const float* syms, int n_frames, const float* n0, int n0_count, int max_trials,
                       uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr)
{
    API_TRY
    if (n_frames > 0 && !syms) return fail(DVBS2_EINVAL, "bad argument");
    return chain_decode_host(h, syms, nullptr, n_frames, n0, n0_count, max_trials, msg, ldpc_ret, bch_corr);
    API_CATCH
}

int dvbs2_chain_decode_llr(dvbs2_chain_t* h, const int8_t* llr, int n_frames, int max_trials, uint8_t* msg, int32_t* ldpc_ret, int32_t* bch_corr)
{
    API_TRY
    if (n_frames > 0 && !llr) return fail(DVBS2_EINVAL, "bad argument");
    return chain_decode_host(h, nullptr, llr, n_frames, nullptr, 0, max_trials, msg, ldpc_ret, bch_corr);
    API_CATCH
}

} // extern "C"
