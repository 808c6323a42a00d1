// c_api_core.hip -- extern "C" boundary (include/dvbs2_fec_hip.h), the entries without a handle: last error, devices, page-locked host
// memory, the FEC parameter and LDPC table queries, the measuring and debugging aids. No exceptions leave the c_api_*.hip files.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>
#include <vector>
#include "host_pipe.h"
#include "fec_tables.h"
#include "ldpc_schedule.h"

using namespace dvbs2;

thread_local std::string dvbs2::g_api_error;

int dvbs2::check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DVBS2_EDEVICE, "no HIP device (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(DVBS2_EINVAL, "device index out of range");
    return DVBS2_OK;
}

extern "C" {

const char* dvbs2_last_error(void) { return g_api_error.c_str(); }

int dvbs2_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dvbs2_host_register(void* p, size_t bytes)
{
    if (!p || !bytes) return fail(DVBS2_EINVAL, "bad argument");
    HCHK(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return DVBS2_OK;
}

int dvbs2_host_is_page_locked(const void* p, size_t bytes) { return host_range_page_locked(p, bytes) ? 1 : 0; }

int dvbs2_host_alloc(void** p, size_t bytes)
{
    if (!p || !bytes) return fail(DVBS2_EINVAL, "bad argument");
    *p = nullptr;
    HCHK(hipHostMalloc(p, bytes, hipHostMallocDefault));
    return DVBS2_OK;
}

int dvbs2_host_free(void* p)
{
    if (!p) return DVBS2_OK;
    HCHK(hipHostFree(p));
    return DVBS2_OK;
}

int dvbs2_host_unregister(void* p)
{
    if (!p) return fail(DVBS2_EINVAL, "bad argument");
    HCHK(hipHostUnregister(p));
    return DVBS2_OK;
}

int dvbs2_get_fec_info(int standard, int framesize, int rate, dvbs2_fec_info_t* out)
{
    if (!out) return fail(DVBS2_EINVAL, "null out");
    FecInfo fi;
    if (!get_fec_info(standard, framesize, rate, &fi)) return fail(DVBS2_EINVAL, "unsupported (standard, framesize, rate)");
    std::memset(out, 0, sizeof(*out));
    out->bch_k = fi.bch_k; out->bch_n = fi.bch_n; out->bch_t = fi.bch_t;
    out->ldpc_k = fi.ldpc_k; out->ldpc_n = fi.ldpc_n;
    if (fi.table) { out->table_k = fi.table->K; std::strncpy(out->table, fi.table->name, sizeof(out->table) - 1); }
    return DVBS2_OK;
}

const char* dvbs2_rate_name(int rate) { return rate_name(rate); }
int dvbs2_rate_from_name(const char* name)
{
    if (!name) return -1;
    for (int r = 0; r < num_rates(); r++) if (!std::strcmp(rate_name(r), name)) return r;
    return -1;
}

const char* dvbs2_ldpc_table_name(int index)
{
    const LdpcTableDesc* t = ldpc_table_at(index);
    return t ? t->name : nullptr;
}

int dvbs2_ldpc_table_info(const char* table, int* n, int* k, int* q, int* links_total, int* conflict_layers)
{
    API_TRY
    LdpcSchedule s;
    if (!compile_ldpc_schedule(find_ldpc_table(table), &s)) return fail(DVBS2_EINVAL, "unknown LDPC table");
    if (n) *n = s.N; if (k) *k = s.K; if (q) *q = s.q;
    if (links_total) *links_total = s.links_total;
    if (conflict_layers) *conflict_layers = s.conflict_layers;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_ldpc_layer_info(const char* table, int layer, int* block, int* groups, int* shifts, int max_entries)
{
    API_TRY
    LdpcSchedule s;
    if (!compile_ldpc_schedule(find_ldpc_table(table), &s)) return fail(DVBS2_EINVAL, "unknown LDPC table");
    if (layer < 0 || layer >= s.q) return fail(DVBS2_EINVAL, "layer out of range");
    const LdpcLayer& L = s.layers[layer];
    if (block) *block = L.block;
    for (int e = 0; e < L.cnt && e < max_entries; e++) {
        const LdpcEntry& en = s.entries[L.entry_off + e];
        if (groups) groups[e] = en.base / 360;
        if (shifts) shifts[e] = (360 - en.rot) % 360;
    }
    return L.cnt;
    API_CATCH
}

int dvbs2_measure_host_copy(int device, size_t bytes, int n_streams, int kind, double* h2d_gbs, double* d2h_gbs)
{
    API_TRY
    if (!bytes || n_streams < 1 || n_streams > 16 || kind < 0 || kind > 2) return fail(DVBS2_EINVAL, "bad argument");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    void* host = nullptr; void* dev = nullptr;
    hipStream_t st[16] = {};
    hipEvent_t e0 = nullptr, e1 = nullptr, done[16] = {};
    int rc = DVBS2_OK;
    bool registered = false;
    auto body = [&]() -> int {
        if (kind == 0) HCHK(hipHostMalloc(&host, bytes));
        else if (kind == 1) {
            // a mapping of its own for the registration (whole pages nothing else lives in; shared anonymous memory: no copy-on-write, no
            // anonymous huge pages under it) -- see dvbs2_host_alloc in the header for why heap memory is not registered here any more
            host = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
            if (host == MAP_FAILED) { host = nullptr; return fail(DVBS2_EDEVICE, "out of host memory"); }
            std::memset(host, 1, bytes);
            HCHK(hipHostRegister(host, bytes, hipHostRegisterDefault));
            registered = true;
        } else {
            host = std::malloc(bytes);
            if (!host) return fail(DVBS2_EDEVICE, "out of host memory");
            std::memset(host, 1, bytes);
        }
        HCHK(hipMalloc(&dev, bytes));
        for (int i = 0; i < n_streams; i++) { HCHK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking)); HCHK(hipEventCreateWithFlags(&done[i], hipEventDisableTiming)); }
        HCHK(hipEventCreate(&e0)); HCHK(hipEventCreate(&e1));
        const size_t part = (bytes / n_streams) & ~(size_t)4095;
        for (int dir = 0; dir < 2; dir++) {
            double best = 0;
            for (int rep = 0; rep < 3; rep++) { // first repetition warms the path
                HCHK(hipDeviceSynchronize());
                HCHK(hipEventRecord(e0, st[0]));
                for (int i = 1; i < n_streams; i++) HCHK(hipStreamWaitEvent(st[i], e0, 0));
                for (int i = 0; i < n_streams; i++) {
                    char* hp = (char*)host + (size_t)i * part; char* dp = (char*)dev + (size_t)i * part;
                    if (dir == 0) HCHK(hipMemcpyAsync(dp, hp, part, hipMemcpyHostToDevice, st[i]));
                    else HCHK(hipMemcpyAsync(hp, dp, part, hipMemcpyDeviceToHost, st[i]));
                    if (i) { HCHK(hipEventRecord(done[i], st[i])); HCHK(hipStreamWaitEvent(st[0], done[i], 0)); }
                }
                HCHK(hipEventRecord(e1, st[0]));
                HCHK(hipEventSynchronize(e1));
                float ms = 0; HCHK(hipEventElapsedTime(&ms, e0, e1));
                if (rep && ms > 0) best = std::max(best, (double)part * n_streams / (ms * 1e-3) / 1e9);
            }
            if (dir == 0) { if (h2d_gbs) *h2d_gbs = best; } else if (d2h_gbs) *d2h_gbs = best;
        }
        return DVBS2_OK;
    };
    rc = body();
    (void)hipDeviceSynchronize();
    for (int i = 0; i < n_streams; i++) { if (st[i]) (void)hipStreamDestroy(st[i]); if (done[i]) (void)hipEventDestroy(done[i]); }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (dev) (void)hipFree(dev);
    if (host) {
        if (kind == 0) (void)hipHostFree(host);
        else if (kind == 1) { if (registered) (void)hipHostUnregister(host); (void)munmap(host, bytes); }
        else std::free(host);
    }
    return rc;
    API_CATCH
}

} // extern "C"

// every SIMD of the device busy with dependent VALU adds; workgroup 0 reports its s_memtime (shader clock) and s_memrealtime (100 MHz) deltas
__global__ void dvbs2_clock_probe_kernel(unsigned long long* out, int n)
{
    unsigned long long r0, r1;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0));
    const unsigned long long t0 = __builtin_readcyclecounter();
    uint32_t a = threadIdx.x;
    for (int i = 0; i < n; i++) asm volatile("v_add_u32 %0, %0, 1\n\tv_add_u32 %0, %0, 1\n\tv_add_u32 %0, %0, 1\n\tv_add_u32 %0, %0, 1" : "+v"(a));
    const unsigned long long t1 = __builtin_readcyclecounter();
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r1));
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; out[2] = a; }
}

extern "C" {

int dvbs2_measure_shader_clock(int device, double* ghz, double* kernel_ms)
{
    API_TRY
    if (!ghz) return fail(DVBS2_EINVAL, "bad argument");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    unsigned long long* d = nullptr; unsigned long long hv[3] = {};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0;
    auto body = [&]() -> int {
        HCHK(hipMalloc(&d, 64));
        HCHK(hipEventCreate(&e0)); HCHK(hipEventCreate(&e1));
        for (int rep = 0; rep < 2; rep++) { // (the first launch lets the clock ramp)
            HCHK(hipEventRecord(e0, nullptr));
            hipLaunchKernelGGL(dvbs2_clock_probe_kernel, dim3(2048), dim3(256), 0, nullptr, d, 300000);
            HCHK(hipEventRecord(e1, nullptr));
            HCHK(hipEventSynchronize(e1));
        }
        HCHK(hipEventElapsedTime(&ms, e0, e1));
        HCHK(hipMemcpy(hv, d, 24, hipMemcpyDeviceToHost));
        return DVBS2_OK;
    };
    const int rc = body();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (rc != DVBS2_OK) return rc;
    if (!hv[1]) return fail(DVBS2_EDEVICE, "clock probe returned nothing");
    *ghz = (double)hv[0] / (double)hv[1] * 0.1; // s_memrealtime counts at 100 MHz
    if (kernel_ms) *kernel_ms = ms;
    return DVBS2_OK;
    API_CATCH
}

int dvbs2_debug_cu_slot_table(int device, int device_key, unsigned long long* table_address, int* nonzero_words)
{
    API_TRY
    if (!table_address) return fail(DVBS2_EINVAL, "bad argument");
    DeviceGuard guard(device);
    if (!guard.ok) return fail(DVBS2_EDEVICE, "hipSetDevice failed");
    std::string e;
    int* t = cu_slot_table(device_key, &e);
    if (!t) return fail(DVBS2_EDEVICE, e);
    *table_address = (unsigned long long)(uintptr_t)t;
    if (nonzero_words) {
        std::vector<int> hv(kCuSlots);
        HCHK(hipMemcpy(hv.data(), t, hv.size() * 4, hipMemcpyDeviceToHost));
        int nz = 0;
        for (int v : hv) nz += v != 0;
        *nonzero_words = nz;
    }
    return DVBS2_OK;
    API_CATCH
}

} // extern "C"
