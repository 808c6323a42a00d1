// ldpc_plan.h -- host-only planner of the LDPC decoder: which build of the sweep kernel a table runs and the records the kernels
// read with scalar loads (format: ldpc_layout.h). Pure integer logic on an LdpcSchedule, no HIP: LdpcDecoderHip's constructor
// uploads what plan_ldpc() returns, tests/test_ldpc_plan.py runs it on the CPU for every table and every override set.
#pragma once
#include <optional>
#include <string>
#include <vector>
#include "ldpc_layout.h"
#include "ldpc_schedule.h"

namespace dvbs2 {

// Environment overrides of the per-table choices (the tests run every build on every table). Unset: the rule.
struct LdpcOverrides {
    std::optional<int> pr, pr_w1, pr_v2, dense, hz2, solo, soft_barrier, v2, v2p, group_sync, group_spin_max, resolve_rounds;
    bool timing = false; // DVBS2_TIMING: the cycle-stamped build and its printouts (diagnostics)
    static LdpcOverrides from_env(); // DVBS2_PR, DVBS2_PR_W1, ... : the only place that reads them, once per handle
};

constexpr int kResolveRounds = 2; // resolution rounds enqueued ahead of time when the group-synchronous stop is off

struct LdpcPlan {
    std::string error; // not empty: the table cannot be decoded (nothing else is valid then)
    LdpcBuild build = LdpcBuild::plain;
    bool pr = false;           // parity-in-records kernel (ldpc_kernel_pr.hpp)
    bool pr_shared_sv = false; // ... with one sign-vector area per workgroup (two do not fit twice into a CU's LDS)
    bool gsync_on = false;     // group-synchronous stop (group_decide)
    int dmax = 0;              // degree class of the kernel: check degrees dmax-7 .. dmax
    int words_per_check = 0;   // message dwords per check
    int resolve_rounds = kResolveRounds, spin_max = kGroupSpinMax;
    size_t lds_bytes = 0, solo_lds_bytes = 0; // dynamic LDS of a workgroup of the build / of a one-frame workgroup of the class
    std::string kernel_name;   // as a profiler shows it, without the argument list
    std::vector<uint32_t> recs, wrecs; // per-layer records (rec_stride) and per-(layer, wave) records (rec_stride_wave)
};
LdpcPlan plan_ldpc(const LdpcSchedule& s, const char* table_name, int group_size, const LdpcOverrides& ov);

} // namespace dvbs2
