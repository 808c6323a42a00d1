// ldpc_inst.hpp -- the instantiation block of one degree class of the classic sweep kernel: ldpc_inst_<dmax>.hip defines
// DVBS2_LDPC_INSTANTIATE as its DMAX and includes this. Which builds exist for the class, their kernels, and the definitions of
// ldpc_variant_prepare / ldpc_variant_launch (ldpc_launch.h).
#pragma once
#ifndef DVBS2_LDPC_INSTANTIATE
#error "define DVBS2_LDPC_INSTANTIATE as the degree class to instantiate"
#endif
#include "ldpc_kernel.hpp"

namespace dvbs2 {

// The cycle-stamped variant (DVBS2_TIMING=1, tools/exp_tables.py) is only built for DMAX = 8 -- the headline tables --
// to keep the build time of the large variants down; elsewhere the request is ignored.
#ifdef DVBS2_TIMING_ALL
template <int DMAX> constexpr bool kTimingBuilt = true; // experiment builds (tools/build_variant.sh timing -DDVBS2_TIMING_ALL)
#else
template <int DMAX> constexpr bool kTimingBuilt = (DMAX == 8);
#endif
// only the degree class 5..12 survives 80 VGPRs (120 B of scratch); the classes of short 5/6 and 8/9 (DMAX 20, 28) spill so
// much that they run 8x slower (measured)
template <int DMAX> constexpr bool kDenseBuilt = (DMAX == 12);
typedef void (*SweepKernel)(const uint32_t*, const uint32_t*, const int8_t*, uint8_t*, uint32_t*, int*, int*, const int*,
                            int, int, int, int, int, int, unsigned long long*, int*, DemapFused);
// The builds of the degree class DMAX, in one place: the kernel of `b`, or null where that build is not compiled for this class.
template <int DMAX> SweepKernel sweep_kernel(LdpcBuild b)
{
    switch (b) {
    case LdpcBuild::plain: return ldpc_layered_kernel<DMAX, false>;
    case LdpcBuild::packed: return ldpc_layered_kernel<DMAX, false, 1, true>;
    case LdpcBuild::solo: if constexpr (kSoloBuilt<DMAX>) return ldpc_layered_kernel<DMAX, false, 1, false, true>; break;
    case LdpcBuild::packed_solo: if constexpr (kSoloBuilt<DMAX>) return ldpc_layered_kernel<DMAX, false, 1, true, true>; break;
    case LdpcBuild::hz2: if constexpr (kHz2Built<DMAX>) return ldpc_layered_kernel<DMAX, false, 1, false, false, true>; break;
    case LdpcBuild::soft: if constexpr (kSoftBuilt<DMAX>) return ldpc_layered_kernel<DMAX, false, 1, false, false, false, true>; break;
    case LdpcBuild::packed_soft: if constexpr (kSoftBuilt<DMAX>) return ldpc_layered_kernel<DMAX, false, 1, true, false, false, true>; break;
    case LdpcBuild::dense: if constexpr (kDenseBuilt<DMAX>) return ldpc_layered_kernel<DMAX, false, 6>; break;
    default: break;
    }
    return nullptr;
}
// the cycle-stamped build (packed nodes, pair workgroups): launched instead of the handle's build while DVBS2_TIMING is set, where it exists
template <int DMAX> SweepKernel timing_kernel()
{
    if constexpr (kTimingBuilt<DMAX>) return ldpc_layered_kernel<DMAX, true, 1, true>;
    return nullptr;
}
template <int DMAX> hipError_t ldpc_variant_prepare(LdpcBuild build, size_t pair_lds_bytes, size_t solo_lds_bytes)
{
    if (!sweep_kernel<DMAX>(build)) return hipErrorInvalidDeviceFunction;
    auto set = [](SweepKernel k, size_t b) { return hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b); };
    hipError_t e = hipSuccess;
    for (int b = 0; b < kLdpcBuilds && e == hipSuccess; b++)
        if (const SweepKernel k = sweep_kernel<DMAX>((LdpcBuild)b)) e = set(k, is_solo((LdpcBuild)b) ? solo_lds_bytes : pair_lds_bytes);
    if (const SweepKernel k = timing_kernel<DMAX>(); k && e == hipSuccess) e = set(k, pair_lds_bytes);
    return e;
}
template <int DMAX> void ldpc_variant_launch(const LdpcLaunch& a)
{
    const SweepKernel tk = a.tdbg ? timing_kernel<DMAX>() : nullptr;
    const SweepKernel k = tk ? tk : sweep_kernel<DMAX>(a.build);
    if (!k) return; // (ldpc_variant_prepare refused such a build)
    const bool solo = !tk && is_solo(a.build);
    hipLaunchKernelGGL(k, solo ? dim3(a.n_frames) : dim3((a.n_frames + 1) / 2), solo ? dim3(kSoloThreads) : dim3(kThreads), a.lds_bytes, a.stream,
                       a.recs, a.wrecs, a.llr_in, a.state, a.msgs, a.iters, a.good, a.target, a.n_frames, a.N, a.K, a.q, a.cap, a.stop_on_good,
                       tk ? a.tdbg : nullptr, solo ? a.cu_slots : nullptr, a.dm);
}
template hipError_t ldpc_variant_prepare<DVBS2_LDPC_INSTANTIATE>(LdpcBuild, size_t, size_t);
template void ldpc_variant_launch<DVBS2_LDPC_INSTANTIATE>(const LdpcLaunch&);

} // namespace dvbs2
