// ldpc_hip.hip -- layered offset-min-sum int8 LDPC belief propagation for DVB-S2/S2X/T2 on gfx950.
//
// What it computes (bit-exact contract): LDPCDecoder<SIMD<int8_t,W>, OffsetMinSumAlgorithm<...,
// NormalUpdate, FACTOR 2>>::operator() of the reference (lib/ldpc_decoder/layered_decoder.hh:143-160,
// lib/ldpc_decoder/algorithms.hh:151-207) for every frame, with the batch-coupled stopping rule of a
// G-frame SIMD batch, followed by the hard decision + MSB-first packing of
// ldpc_decoder_bb_impl::general_work (lib/ldpc_decoder_bb_impl.cc:432-442).
//
// Mapping (MI355X-first, not a translation of the lane-per-frame SIMD decoder):
//   * one FECFRAME per workgroup of 6 wavefronts; thread j (< 360) owns check node (layer i, lane j)
//     of every layer, i.e. one row of each circulant;
//   * the frame's N LLRs live in LDS for the whole decode (offset-binary bytes, parity part permuted
//     to [layer][lane]); a table entry (group g, shift s) is a rotated contiguous 360-byte window of it;
//   * the check-to-bit messages are private to the owning thread: they stream through L2/Infinity
//     Cache as coalesced dwords (4 int8 messages per dword), never through LDS;
//   * layers with two entries of the same group (sequential-order hazard of the reference's strictly
//     ordered update) are processed in ascending lane blocks of B_i (ldpc_schedule.h).
#include "ldpc_hip.h"
#include "ldpc_plan.h"
#include "ldpc_launch.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace dvbs2 {

// Per-group stopping rule of one reference SIMD batch: while (bad(any lane) && --trials >= 0) update(all lanes)
// (layered_decoder.hh:153). After a pass, every frame f sits at iters[f] updates with good[f] known there.
__global__ void ldpc_group_targets_kernel(const int* iters, const int* good, int* target, int* flag,
                                          int* ret, int n_groups, int G, int n_frames, int cap)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const int f0 = g * G, f1 = min(f0 + G, n_frames);
    int T = 0;
    for (int f = f0; f < f1; f++) T = max(T, iters[f]);
    bool aligned = true, all_good = true;
    for (int f = f0; f < f1; f++) {
        if (iters[f] != T) aligned = false;
        else if (!good[f]) all_good = false;
    }
    int tgt = T;
    bool unresolved = false;
    if (!aligned) unresolved = true;               // bring the early stoppers up to T, then look again
    else if (!all_good && T < cap) { tgt = T + 1; unresolved = true; }
    for (int f = f0; f < f1; f++) target[f] = tgt;
    if (unresolved) atomicAdd(flag, 1);
    else if (ret) ret[g] = all_good ? cap - T : -1;
}

// Hard decision + MSB-first packing (ldpc_decoder_bb_impl.cc:432-442) and optional soft output
// (the llr_pdu payload, :422-429), undoing the parity permutation (layered_decoder.hh:155-157).
// One thread per eight LLRs = one output byte. The information part of the state is in natural order: one 8-byte load, the
// sign bits gathered with a multiply (bits 7, 15, 23, 31 of a dword -> four adjacent bits), one byte stored (round 2 read
// byte by byte: 0.49 ms per 4096 normal frames, 1.3 % of a 50-update batch). The parity part (whole-codeword output and the
// soft output only) is gathered through the permutation pty[360 i + j] = parity[q j + i].
__device__ __forceinline__ uint32_t neg_bits4(uint32_t w) // offset-binary bytes b0..b3 -> (b0 < 0x80) << 3 | ... | (b3 < 0x80)
{
    const uint32_t m = (~w & 0x80808080u) >> 7;            // one bit per byte, at bits 0, 8, 16, 24
    return ((m * 0x08040201u) >> 24) & 0xfu;               // b0 -> bit 3, b1 -> bit 2, b2 -> bit 1, b3 -> bit 0
}
__global__ void ldpc_finalize_kernel(const uint8_t* state, uint8_t* bits, int8_t* llr_out,
                                     int N, int K, int q, int out_bytes)
{
    const int f = blockIdx.y;
    const uint8_t* s = state + (size_t)f * N;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= N / 8 || (!llr_out && b >= out_bytes)) return;
    uint2 v;
    if (8 * b < K) v = *reinterpret_cast<const uint2*>(s + 8 * b); // K % 8 == 0
    else {
        uint32_t w[2] = { 0, 0 };
        int r = 8 * b - K, jq = r / q, iq = r - jq * q;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            w[k >> 2] |= (uint32_t)s[K + kM * iq + jq] << (8 * (k & 3));
            if (++iq == q) { iq = 0; ++jq; }
        }
        v = make_uint2(w[0], w[1]);
    }
    if (llr_out) *reinterpret_cast<uint2*>(llr_out + (size_t)f * N + 8 * b) = make_uint2(v.x ^ 0x80808080u, v.y ^ 0x80808080u);
    if (bits && b < out_bytes) bits[(size_t)f * out_bytes + b] = (uint8_t)((neg_bits4(v.x) << 4) | neg_bits4(v.y));
}

// The per-CU pattern counters of the one-frame builds, ONE array per device for all handles (see the constructor): keyed by the device id,
// allocated on the CURRENT device and zeroed before its pointer is published, never freed (the counts survive the handles; they are not
// valid across hipDeviceReset()). A function of its own so that the table can be exercised with device keys a one-GPU box does not have
// (dvbs2_debug_cu_slot_table, tests/test_ldpc_gpu.py::test_cu_slot_table_is_per_device).
int* cu_slot_table(int device_key, std::string* err)
{
    static std::mutex mu;
    static std::vector<std::pair<int, int*>> per_device;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& e : per_device) if (e.first == device_key) return e.second;
    int* slots = nullptr;
    if (hipMalloc(&slots, kCuSlots * 4) != hipSuccess) { if (err) *err = "hipMalloc of the per-CU counters failed"; return nullptr; }
    if (memset_done(slots, 0, kCuSlots * 4) != hipSuccess) { (void)hipFree(slots); if (err) *err = "hipMemset of the per-CU counters failed"; return nullptr; }
    per_device.push_back({ device_key, slots });
    return slots;
}

namespace {
// the entry points of one sweep kernel family: the classic kernel per degree class (ldpc_inst_<dmax>.hip), parity in records (ldpc_inst_pr.hip)
struct SweepOps { hipError_t (*prepare)(LdpcBuild, size_t pair_lds_bytes, size_t solo_lds_bytes); void (*launch)(const LdpcLaunch&); };
hipError_t pr_prepare(LdpcBuild b, size_t lds_bytes, size_t) { return ldpc_pr_prepare(b, lds_bytes); }
const SweepOps& sweep_ops(bool pr, int dmax)
{
    static const SweepOps kPr = { pr_prepare, ldpc_pr_launch };
    static const SweepOps kClassic[8] = {
        { ldpc_variant_prepare<4>, ldpc_variant_launch<4> },   { ldpc_variant_prepare<8>, ldpc_variant_launch<8> },
        { ldpc_variant_prepare<12>, ldpc_variant_launch<12> }, { ldpc_variant_prepare<16>, ldpc_variant_launch<16> },
        { ldpc_variant_prepare<20>, ldpc_variant_launch<20> }, { ldpc_variant_prepare<24>, ldpc_variant_launch<24> },
        { ldpc_variant_prepare<28>, ldpc_variant_launch<28> }, { ldpc_variant_prepare<32>, ldpc_variant_launch<32> },
    };
    return pr ? kPr : kClassic[dmax / 4 - 1];
}
} // namespace

LdpcDecoderHip::LdpcDecoderHip(const LdpcTableDesc* table, int out_bits_message, int group_size, int max_frames, int device)
    : DeviceStage(device), out_bits_message_(out_bits_message), G_(group_size), max_frames_(max_frames)
{
    if (!compile_ldpc_schedule(table, &sched_)) { err_.argument("unknown or inconsistent LDPC table"); return; }
    if (G_ < 1 || max_frames_ < 1 || max_frames_ > 65535) { err_.argument("bad group_size/max_frames (max_frames 1..65535: frames are one launch dimension)"); return; }
    if (out_bits_message_ <= 0 || out_bits_message_ > sched_.N || out_bits_message_ % 8) { err_.argument("bad message length"); return; }
    // which build of the sweep kernel, and the records laid out for it: the host-only planner (ldpc_plan.cpp)
    const LdpcOverrides ov = LdpcOverrides::from_env();
    const LdpcPlan plan = plan_ldpc(sched_, table->name, G_, ov);
    if (!plan.error.empty()) { err_.argument(plan.error); return; }
    build_ = plan.build; pr_ = plan.pr; pr_shared_sv_ = plan.pr_shared_sv; gsync_on_ = plan.gsync_on; dmax_ = plan.dmax; words_per_check_ = plan.words_per_check;
    resolve_rounds_ = plan.resolve_rounds; lds_bytes_ = plan.lds_bytes; kname_ = plan.kernel_name;

    DeviceGuard dev_guard(device_); // the caller's current device is restored when the constructor returns (device_guard.h)
    if (!dev_guard.ok) { err_.device("hipSetDevice failed"); return; }
    HIP_OK_AS("hipMalloc(&d_recs_alloc_, (plan.recs.size() + kRecHeaderWords) * 4)", alloc(&d_recs_alloc_, plan.recs.size() + kRecHeaderWords)); // header (group-synchronous stop, filled below) + records
    d_recs_ = d_recs_alloc_ + kRecHeaderWords;
    HIP_OK(hipMemcpy(d_recs_, plan.recs.data(), plan.recs.size() * 4, hipMemcpyHostToDevice));
    HIP_OK_AS("hipMalloc(&d_wrecs_, plan.wrecs.size() * 4)", alloc(&d_wrecs_, plan.wrecs.size()));
    HIP_OK(hipMemcpy(d_wrecs_, plan.wrecs.data(), plan.wrecs.size() * 4, hipMemcpyHostToDevice));
    HIP_OK_AS("hipMalloc(&d_state_, (size_t)max_frames_ * sched_.N)", alloc(&d_state_, (size_t)max_frames_ * sched_.N));
    HIP_OK_AS("hipMalloc(&d_msgs_, (size_t)max_frames_ * sched_.q * words_per_check_ * kMsgStride * 4)", alloc(&d_msgs_, (size_t)max_frames_ * sched_.q * words_per_check_ * kMsgStride));
    HIP_OK_AS("hipMalloc(&d_iters_, (size_t)max_frames_ * 4)", alloc(&d_iters_, (size_t)max_frames_));
    HIP_OK_AS("hipMalloc(&d_good_, (size_t)max_frames_ * 4)", alloc(&d_good_, (size_t)max_frames_));
    HIP_OK_AS("hipMalloc(&d_target_, (size_t)max_frames_ * 4)", alloc(&d_target_, (size_t)max_frames_));
    if (gsync_on_) { // group-synchronous stop (ldpc_plan.cpp, group_decide): its words and the header in front of the records
        HIP_OK_AS("hipMalloc(&d_gsync_, (size_t)(max_frames_ + 64) * 4)", alloc(&d_gsync_, (size_t)(max_frames_ + 64))); // one status word per frame (group_decide)
        const unsigned long long a = (unsigned long long)d_iters_, b = (unsigned long long)d_gsync_;
        const uint32_t hd[kRecHeaderWords] = { (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)G_, (uint32_t)plan.spin_max, 0, 0 };
        HIP_OK(hipMemcpy(d_recs_alloc_, hd, sizeof(hd), hipMemcpyHostToDevice));
    }
    HIP_OK_AS("hipMalloc(&d_flag_, 4 * kSlots)", alloc(&d_flag_, kSlots));
    HIP_OK(hipHostMalloc(&h_flag_, 4 * kSlots));
    HIP_OK(hipEventCreate(&ev0_));
    HIP_OK(hipEventCreate(&ev1_));
    if (ov.timing) { HIP_OK_AS("hipMalloc(&d_tdbg_, ((size_t)max_frames_ * 48 + 512) * 8)", alloc(&d_tdbg_, (size_t)max_frames_ * 48 + 512)); HIP_OK(memset_done(d_tdbg_, 0, ((size_t)max_frames_ * 48 + 512) * 8)); }
    if (is_solo(build_)) {
        // The per-CU pattern counters of the one-frame builds are shared by ALL handles of a device: two workgroups on a CU take
        // complementary wave patterns through them, whichever launch (handle, stream) they belong to. With one array per handle two
        // pipelined handles both chose pattern 0 on every CU: 4,4,2,2 working waves per SIMD instead of 3,3,3,3 and the operating point
        // through two handles fell from 0.92 to 0.71 of the proportional rate (round 4). Allocated once per device, never freed.
        // Keyed by the device this constructor actually runs on (hipGetDevice behind the guard), one entry per device ever seen; the
        // array is zeroed BEFORE its pointer is published. The counts survive the handles (a kernel gives its slot back when it ends);
        // they are not valid across hipDeviceReset().
        int dv = -1;
        HIP_OK(hipGetDevice(&dv));
        std::string e;
        int* slots = cu_slot_table(dv, &e);
        if (!slots) { err_.device(e); return; }
        d_cu_slots_ = slots;
    }
    if (!hip_ok(sweep_ops(pr_, dmax_).prepare(build_, lds_bytes_, plan.solo_lds_bytes), "sweep_ops(pr_, dmax_).prepare(build_, lds_bytes_, plan.solo_lds_bytes)", err_, kArgument)) return; // (device failure, kArgument: notes/stage_error_codes.md)
}

LdpcDecoderHip::~LdpcDecoderHip()
{
    DeviceGuard dev_guard(device_); // (the device buffers: ~DeviceStage)
    if (h_flag_) (void)hipHostFree(h_flag_);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
}

void LdpcDecoderHip::launch_sweep(const int8_t* in, bool resume, int stop_on_good, int n_frames, int max_trials, int frame_base, hipStream_t stream, const DemapFused* dm)
{
    if (profiling_) (void)hipEventRecord(ev0_, stream);
    const size_t fb = (size_t)frame_base;
    LdpcLaunch la;
    la.recs = d_recs_; la.wrecs = d_wrecs_; la.llr_in = in; la.state = d_state_ + fb * sched_.N;
    la.msgs = d_msgs_ + fb * sched_.q * words_per_check_ * kMsgStride;
    la.iters = d_iters_ + fb; la.good = d_good_ + fb; la.target = resume ? d_target_ + fb : nullptr;
    const bool gs = gsync_on_ && !resume && stop_on_good; // group-synchronous stop (kFlagGroupSync); its words start from zero
    if (gs) (void)hipMemsetAsync(d_gsync_ + frame_base, 0, (size_t)n_frames * 4, stream); // (frame_base is a multiple of the group size: enqueue())
    const bool soft_bar = build_ == LdpcBuild::soft || build_ == LdpcBuild::packed_soft;
    la.n_frames = n_frames; la.N = sched_.N; la.K = sched_.K; la.q = sched_.q; la.cap = max_trials;
    la.stop_on_good = stop_on_good | (soft_bar ? kFlagSoftBarrier : 0) | (gs ? kFlagGroupSync : 0) | (pr_ && pr_shared_sv_ ? kFlagPrSharedSv : 0);
    la.tdbg = d_tdbg_; la.lds_bytes = is_solo(build_) ? half_lds_bytes(sched_.N) : lds_bytes_; la.stream = stream;
    la.build = build_; la.cu_slots = d_cu_slots_;
    la.dm = DemapFused{};
    if (dm && !resume) la.dm = *dm;
    sweep_ops(pr_, dmax_).launch(la);
    if (profiling_ && !resume) { // the first pass is the dominant launch; timing it serialises the stream (bench.py's roofline leg only)
        (void)hipEventRecord(ev1_, stream);
        (void)hipEventSynchronize(ev1_);
        float ms = 0; (void)hipEventElapsedTime(&ms, ev0_, ev1_);
        prof_ms_ += ms; prof_launches_++;
    }
}

void LdpcDecoderHip::launch_targets(int n_frames, int max_trials, int frame_base, int32_t* d_ret, int slot, hipStream_t stream)
{
    const int n_groups = (n_frames + G_ - 1) / G_;
    (void)hipMemsetAsync(d_flag_ + slot, 0, 4, stream);
    hipLaunchKernelGGL(ldpc_group_targets_kernel, dim3((n_groups + 127) / 128), dim3(128), 0, stream,
                       d_iters_ + frame_base, d_good_ + frame_base, d_target_ + frame_base, d_flag_ + slot, d_ret, n_groups, G_, n_frames, max_trials);
}

void LdpcDecoderHip::launch_finalize(const Pending& p)
{
    if (!p.bits && !p.llr_out) return; // nobody asked for packed bits or LLRs (chain: the BCH stage reads the state)
    const int out_bytes = (p.out_mode ? out_bits_message_ : sched_.N) / 8;
    const int items = p.llr_out ? sched_.N / 8 : out_bytes; // one thread per eight LLRs; without the soft output only the bytes asked for
    hipLaunchKernelGGL(ldpc_finalize_kernel, dim3((items + 255) / 256, p.n_frames), dim3(256), 0, p.stream,
                       d_state_ + (size_t)p.frame_base * sched_.N, p.bits, p.llr_out, sched_.N, sched_.K, sched_.q, out_bytes);
}

// DVBS2_TIMING: waits for the first pass and prints the cycle stamps its cycle-stamped build left (diagnostics; -1: a HIP call failed)
int LdpcDecoderHip::dump_timing(int n_frames, int max_trials, hipStream_t stream)
{
    HIP_RET(hipStreamSynchronize(stream));
    if (getenv("DVBS2_TIMING_LAYERS")) { // cycles per layer of frame 0, wave 0 (sum over the sweeps so far)
        std::vector<unsigned long long> hl(sched_.q);
        HIP_RET(hipMemcpy(hl.data(), d_tdbg_ + (size_t)n_frames * 48, hl.size() * 8, hipMemcpyDeviceToHost));
        {   // hazard-node phases (check_node_hazard, DVBS2_PH): wave 0 = chain heads / walker, wave 5 = body rows
            std::vector<unsigned long long> hp(32);
            HIP_RET(hipMemcpy(hp.data(), d_tdbg_ + (size_t)n_frames * 48 + 256, 32 * 8, hipMemcpyDeviceToHost));
            static const char* const nm[8] = { "P1", "heads", "barrier", "publish+barrier", "walk", "barrier", "steps/finish+barrier", "merge+P3" };
            for (int w = 0; w < 2; w++) {
                fprintf(stderr, "  hazard phases wave %d (cycles/sweep):", w ? 5 : 0);
                for (int k = 0; k < 8; k++) fprintf(stderr, " %s %.0f", nm[k], (double)hp[16 * w + k] / std::max(1, max_trials));
                fprintf(stderr, "\n");
            }
        }
        HIP_RET(hipMemset(d_tdbg_ + (size_t)n_frames * 48, 0, 512 * 8));
        for (int i = 0; i < sched_.q; i++) fprintf(stderr, "  layer %3d block %3d nconf %d deg %2d: %8.0f cycles/sweep\n", i, sched_.layers[i].block, sched_.layers[i].n_conflict, sched_.layers[i].cnt + 2, (double)hl[i] / std::max(1, max_trials));
    }
    std::vector<unsigned long long> h((size_t)n_frames * 48);
    HIP_RET(hipMemcpy(h.data(), d_tdbg_, h.size() * 8, hipMemcpyDeviceToHost));
    double a[8] = {0};
    for (size_t r = 0; r < (size_t)n_frames * 6; r++) for (int c = 0; c < 8; c++) a[c] += (double)h[r * 8 + c];
    const double nr = (double)n_frames * 6;
    if (getenv("DVBS2_TIMING_WAVES")) {
        for (int w = 0; w < 6; w++) {
            double b[8] = {0};
            for (size_t fr = 0; fr < (size_t)n_frames; fr++) for (int c = 0; c < 8; c++) b[c] += (double)h[(fr * 6 + w) * 8 + c];
            fprintf(stderr, "  wave %d: sweep %.0f barrier %.0f body %.0f conflict %.0f\n", w, b[2] / n_frames, b[3] / n_frames, b[4] / n_frames, b[5] / n_frames);
        }
    }
    fprintf(stderr, "[timing, shader-clock cycles per wave avg] load %.0f synd %.0f sweep %.0f (barrier %.0f body %.0f conflict-layers %.0f) iters %.1f synd-step1 %.0f\n", a[0]/nr, a[1]/nr, a[2]/nr, a[3]/nr, a[4]/nr, a[5]/nr, a[6]/nr, a[7]/nr);
    return 0;
}

int LdpcDecoderHip::enqueue(const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode, uint8_t* d_bits_out, int8_t* d_llr_out,
                            int32_t* d_ret, hipStream_t stream, int slot, int frame_base, const DemapFused* dm)
{
    if (!ok()) return -1;
    call_err_ = {};
    if (slot < 0 || slot >= kSlots) { call_err_.device("bad slot"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (pend_[slot].active) { call_err_.device("slot busy: finish() the previous decode first"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_frames < 0 || frame_base < 0 || frame_base + n_frames > max_frames_) { call_err_.device("n_frames exceeds max_frames"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (frame_base % 2 || (frame_base && frame_base % G_)) { call_err_.device("frame_base must be a multiple of the group size and even"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (max_trials < 0) { call_err_.device("max_trials < 0"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    Pending& p = pend_[slot];
    // a call that fails below leaves the slot free again (the handle stays usable: "a failed call does not disable the handle")
    // (and nothing of it stays in flight: kernels and copies already queued on the stream are waited for before the slot is given up)
    struct Release { Pending& p; bool armed = true, launched = false; ~Release() { if (armed) { if (launched) (void)hipStreamSynchronize(p.stream); p.active = false; } } } release{ p };
    p.active = true; p.n_frames = n_frames; p.max_trials = max_trials; p.out_mode = out_mode; p.frame_base = frame_base;
    p.bits = d_bits_out; p.llr_out = d_llr_out; p.ret = d_ret; p.stream = stream;
    h_flag_[slot] = 0;
    if (n_frames == 0) { release.armed = false; return 0; }
    Entry on(*this);
    if (!on.ok) return -1;
    if (dm && dm->mode && pr_) { call_err_.device("this sweep kernel does not demap while loading"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    release.launched = true;
    launch_sweep(d_llr_in, false, 1, n_frames, max_trials, frame_base, stream, dm);
    if (d_tdbg_ && dump_timing(n_frames, max_trials, stream)) return -1;
    // group resolution on the device: no host round trip (a resume launch whose frames are all at their target costs a few
    // microseconds: its workgroups read two counters and leave)
    for (int r = 0; r < resolve_rounds_; r++) {
        launch_targets(n_frames, max_trials, frame_base, d_ret, slot, stream);
        launch_sweep(nullptr, true, 0, n_frames, max_trials, frame_base, stream);
    }
    launch_targets(n_frames, max_trials, frame_base, d_ret, slot, stream);
    launch_finalize(p);
    HIP_RET(hipMemcpyAsync(h_flag_ + slot, d_flag_ + slot, 4, hipMemcpyDeviceToHost, stream));
    HIP_RET(hipGetLastError());
    release.armed = false;
    return 0;
}

int LdpcDecoderHip::finish(int slot)
{
    if (!ok()) return -1;
    if (slot < 0 || slot >= kSlots) { call_err_.device("bad slot"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    Pending& p = pend_[slot];
    if (!p.active) return 0;
    p.active = false;
    if (p.n_frames == 0) return 0;
    Entry on(*this);
    if (!on.ok) return -1;
    HIP_RET(hipStreamSynchronize(p.stream));
    if (h_flag_[slot] == 0) return 0;
    struct Drain { hipStream_t st; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(st); } } drain{ p.stream }; // a failing round leaves nothing in flight
    for (int round = 0; h_flag_[slot] != 0; round++) { // the rare leftovers, one host round trip each
        if (round > 2 * p.max_trials + 2) { call_err_.device("group resolution did not converge"); return -1; }
        fallback_rounds_++;
        launch_sweep(nullptr, true, 0, p.n_frames, p.max_trials, p.frame_base, p.stream);
        launch_targets(p.n_frames, p.max_trials, p.frame_base, p.ret, slot, p.stream);
        HIP_RET(hipMemcpyAsync(h_flag_ + slot, d_flag_ + slot, 4, hipMemcpyDeviceToHost, p.stream));
        HIP_RET(hipStreamSynchronize(p.stream));
    }
    launch_finalize(p);
    HIP_RET(hipGetLastError());
    HIP_RET(hipStreamSynchronize(p.stream));
    drain.armed = false;
    return 1; // outputs were rewritten after the stream's first completion
}

void LdpcDecoderHip::abort_all()
{
    DeviceGuard dev_guard(device_);
    for (Pending& p : pend_) {
        if (p.active && p.n_frames > 0 && dev_guard.ok) (void)hipStreamSynchronize(p.stream);
        p.active = false;
    }
}

int LdpcDecoderHip::decode_device(const int8_t* d_llr_in, int n_frames, int max_trials, int out_mode,
                                  uint8_t* d_bits_out, int8_t* d_llr_out, int32_t* d_ret, hipStream_t stream)
{
    if (enqueue(d_llr_in, n_frames, max_trials, out_mode, d_bits_out, d_llr_out, d_ret, stream, 0, 0)) return -1;
    return finish(0) < 0 ? -1 : 0;
}

} // namespace dvbs2
