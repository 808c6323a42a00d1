// ldpc_launch.h -- host-side launch interface of the sweep kernels: what ldpc_hip.hip needs to prepare and launch a build, and no device
// code. The classic kernel is defined per degree class in ldpc_inst_<dmax>.hip (ldpc_inst.hpp), parity in records in ldpc_inst_pr.hip
// (ldpc_kernel_pr.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "demap_math.hpp"
#include "ldpc_layout.h"

namespace dvbs2 {

// ---- one kernel variant of the classic kernel (defined in ldpc_inst_<dmax>.hip) ----
struct LdpcLaunch {
    const uint32_t* recs; const uint32_t* wrecs; const int8_t* llr_in; uint8_t* state; uint32_t* msgs; int* iters; int* good; const int* target;
    int n_frames, N, K, q, cap, stop_on_good; unsigned long long* tdbg /*non-null: the cycle-stamped build where it exists*/;
    DemapFused dm;
    size_t lds_bytes; hipStream_t stream;
    LdpcBuild build;
    int* cu_slots;
};
// prepare: sets the dynamic-LDS limit of every build of the class (one-frame builds take solo_lds_bytes); fails when `build` is not one of them
template <int DMAX> hipError_t ldpc_variant_prepare(LdpcBuild build, size_t pair_lds_bytes, size_t solo_lds_bytes);
template <int DMAX> void ldpc_variant_launch(const LdpcLaunch& a);
template <int DMAX> constexpr bool kSoloBuilt = (DMAX <= kSoloMaxDmax);
template <int DMAX> constexpr bool kHz2Built = (DMAX >= 12);
template <int DMAX> constexpr bool kSoftBuilt = (DMAX >= 20); // pays where layers are long and barriers few (measured: S2X B10, B20, B21, B24)
// (Plain builds with the packed chain node measured SLOWER than the plain build's own lane chain -- B4 107.8 k vs 109.8 k, B5 57.9 k vs
// 62.2 k frames/s -- although its ordered steps cost a third: the node's register state hurts the rest of the kernel. Not built.)

// the parity-in-records builds (LdpcBuild::pr, pr_w1, pr_packed; defined in ldpc_inst_pr.hip); prepare fails when `build` is not one of them
hipError_t ldpc_pr_prepare(LdpcBuild build, size_t lds_bytes);
void ldpc_pr_launch(const LdpcLaunch& a);

} // namespace dvbs2
