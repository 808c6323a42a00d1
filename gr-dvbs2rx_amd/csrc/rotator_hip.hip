// rotator_hip.hip -- see rotator_hip.h.
#include "rotator_hip.h"
#include "rotator_math.hpp"
#include "rotator_turns.h"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

namespace dvbs2 {

namespace {

constexpr int kSegs = 8; // segments one launch takes; a call with more is cut into launches
struct RotSegs {
    int start[kSegs];      // relative to the launch, ascending; unused entries INT_MAX
    uint64_t phase[kSegs], inc[kSegs];
};

template <bool kMulti> __device__ inline uint64_t phase_at(const RotSegs& g, int i)
{
    int st = g.start[0];
    uint64_t p = g.phase[0], inc = g.inc[0];
    if (kMulti) {
#pragma unroll
        for (int k = 1; k < kSegs; k++) if (i >= g.start[k]) { st = g.start[k]; p = g.phase[k]; inc = g.inc[k]; }
    }
    return p + (uint64_t)(uint32_t)(i - st) * inc;
}

// Streaming, grid-stride, two symbols (16 bytes) per lane and step where input and output allow the same 16-byte phase; every thread
// reads and writes its own symbols only, so out == in is safe. No __restrict__ for that reason.
template <bool kMulti> __global__ __launch_bounds__(256) void rotator_kernel(const float2* in, float2* out, int n, RotSegs g)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
    const bool vec = (((uintptr_t)in ^ (uintptr_t)out) & 15) == 0;
    if (!vec) {
        for (int i = tid; i < n; i += nthreads) out[i] = rotate_one(in[i], phase_at<kMulti>(g, i));
        return;
    }
    const int head = (int)(((uintptr_t)in >> 3) & 1) < n ? (int)(((uintptr_t)in >> 3) & 1) : n; // one symbol up to the 16-byte boundary
    const int npairs = (n - head) >> 1;
    const float4* in4 = reinterpret_cast<const float4*>(in + head);
    float4* out4 = reinterpret_cast<float4*>(out + head);
    for (int j = tid; j < npairs; j += nthreads) {
        const int i = head + 2 * j;
        const float4 v = in4[j];
        const float2 a = rotate_one(make_float2(v.x, v.y), phase_at<kMulti>(g, i));
        const float2 b = rotate_one(make_float2(v.z, v.w), phase_at<kMulti>(g, i + 1));
        out4[j] = make_float4(a.x, a.y, b.x, b.y);
    }
    if (tid == 0) {
        if (head) out[0] = rotate_one(in[0], phase_at<kMulti>(g, 0));
        const int last = head + 2 * npairs;
        if (last < n) out[last] = rotate_one(in[last], phase_at<kMulti>(g, last));
    }
}

// the yardstick of rotator_measure: the same 16 bytes per lane and step, the same grid, nothing in between
__global__ __launch_bounds__(256) void copy16_kernel(const float4* __restrict__ in, float4* __restrict__ out, int n4)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n4; j += gridDim.x * blockDim.x) out[j] = in[j];
}

} // namespace

int rotator_measure(int device, int n_syms, int regions, double* rot_ms, double* copy_ms, std::string* err)
{
    if (n_syms < 2 || regions < 1 || regions > 64) { *err = "bad argument"; return kArgument; }
    DeviceGuard dev_guard(device);
    RotatorHip rot(0.0123, device);
    float *d_in = nullptr, *d_out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const size_t bytes = (size_t)n_syms * 8;
    std::vector<float> tr, tc;
    bool good = dev_guard.ok && hipMalloc(&d_in, bytes) == hipSuccess && hipMalloc(&d_out, bytes) == hipSuccess &&
                hipMemset(d_in, 0x3c, bytes) == hipSuccess && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    const int n4 = n_syms / 2, blocks = (int)std::min<int64_t>(((int64_t)n4 + 256) / 256, 4096);
    for (int r = -1; good && r < regions; r++) { // region -1 warms both up
        float ms = 0.0f;
        good = hipEventRecord(e0, nullptr) == hipSuccess && rot.rotate_device(d_in, n_syms, d_out, nullptr) == 0 &&
               hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (good && r >= 0) tr.push_back(ms);
        if (!good) break;
        good = hipEventRecord(e0, nullptr) == hipSuccess;
        hipLaunchKernelGGL(copy16_kernel, dim3(blocks), dim3(256), 0, nullptr, reinterpret_cast<const float4*>(d_in), reinterpret_cast<float4*>(d_out), n4);
        good = good && hipGetLastError() == hipSuccess && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
               hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (good && r >= 0) tc.push_back(ms);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d_in); (void)hipFree(d_out);
    if (!good) { *err = "device setup or launch failed"; return kDevice; }
    std::sort(tr.begin(), tr.end()); std::sort(tc.begin(), tc.end());
    *rot_ms = tr[tr.size() / 2]; *copy_ms = tc[tc.size() / 2];
    return 0;
}

RotatorHip::RotatorHip(double phase_inc, int device) : DeviceStage(device), inc0_(phase_inc)
{
    if (!std::isfinite(phase_inc)) { err_.argument("phase_inc must be finite"); return; }
    reset();
}

void RotatorHip::reset()
{
    call_err_ = {};
    counter_ = 0; phase_ = 0; inc_ = rotator_inc_turns(inc0_);
    queue_.clear();
}

int RotatorHip::set_phase_inc(double inc)
{
    call_err_ = {};
    if (!std::isfinite(inc)) { call_err_.argument("phase_inc must be finite"); return -1; }
    inc_ = rotator_inc_turns(inc);
    return 0;
}

int RotatorHip::schedule(int64_t offset, double inc)
{
    call_err_ = {};
    if (!std::isfinite(inc)) { call_err_.argument("phase_inc must be finite"); return -1; }
    if (offset < 0) { call_err_.argument("offset must not be negative"); return -1; }
    // after every queued update of the same or a smaller offset: equal offsets keep their scheduling order
    auto it = std::upper_bound(queue_.begin(), queue_.end(), offset, [](int64_t o, const Update& u) { return o < u.offset; });
    queue_.insert(it, Update{ offset, inc });
    return 0;
}

// lib/rotator_cc_impl.cc:83-125 over the samples [counter_, counter_ + n)
void RotatorHip::advance(int64_t n, std::vector<Segment>* segs)
{
    int64_t done = 0;
    size_t used = 0;
    while (used < queue_.size()) {
        const Update& u = queue_[used];
        if (u.offset < counter_ + done) { used++; continue; } // not processed on time: dropped
        if (u.offset >= counter_ + n) break;                  // for a later call
        const int64_t items = u.offset - counter_ - done;
        if (items > 0 && segs) segs->push_back(Segment{ done, phase_, inc_ });
        phase_ += (uint64_t)items * inc_;
        done += items;
        inc_ = rotator_inc_turns(u.inc);
        used++;
    }
    queue_.erase(queue_.begin(), queue_.begin() + used);
    if (n - done > 0 && segs) segs->push_back(Segment{ done, phase_, inc_ });
    phase_ += (uint64_t)(n - done) * inc_;
    counter_ += n;
}

int RotatorHip::seek(int64_t n)
{
    if (!ok()) return -1;
    call_err_ = {};
    if (n < 0 || n > INT64_MAX - counter_) { call_err_.argument("seek distance out of range"); return -1; }
    advance(n, nullptr);
    return 0;
}

int RotatorHip::rotate_device(const float* d_in, int n_syms, float* d_out, hipStream_t stream)
{
    Entry on(*this);
    if (!on.ok) return -1;
    if (n_syms < 0 || (int64_t)n_syms > INT64_MAX - counter_) { call_err_.device("n_syms out of range"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    if (n_syms == 0) return 0;
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 7) { call_err_.device("symbol buffers must be 8-byte aligned"); return -1; } // (argument text, kDevice: notes/stage_error_codes.md)
    std::vector<Segment> segs;
    advance(n_syms, &segs);
    const float2* in = reinterpret_cast<const float2*>(d_in);
    float2* out = reinterpret_cast<float2*>(d_out);
    for (size_t s = 0; s < segs.size(); s += kSegs) {
        const size_t cnt = std::min((size_t)kSegs, segs.size() - s);
        const int64_t a = segs[s].start, b = s + cnt < segs.size() ? segs[s + cnt].start : (int64_t)n_syms;
        RotSegs g;
        for (int k = 0; k < kSegs; k++) {
            const bool on = (size_t)k < cnt;
            g.start[k] = on ? (int)(segs[s + k].start - a) : INT_MAX;
            g.phase[k] = on ? segs[s + k].phase : 0;
            g.inc[k] = on ? segs[s + k].inc : 0;
        }
        const int n = (int)(b - a);
        const int blocks = (int)std::min<int64_t>(((int64_t)n / 2 + 256) / 256, 4096);
        if (cnt == 1) hipLaunchKernelGGL(rotator_kernel<false>, dim3(blocks), dim3(256), 0, stream, in + a, out + a, n, g);
        else hipLaunchKernelGGL(rotator_kernel<true>, dim3(blocks), dim3(256), 0, stream, in + a, out + a, n, g);
        if (launched("rotator kernel launch")) return -1;
    }
    return 0;
}

} // namespace dvbs2
