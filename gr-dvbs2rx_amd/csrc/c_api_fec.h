// c_api_fec.h -- the LDPC, BCH and demapper handles, which the chain (c_api_chain.hip) reaches into. Internal, not installed.
#pragma once
#include "host_pipe.h"
#include "bch_hip.h"
#include "demap_hip.h"

struct dvbs2_ldpc {
    dvbs2::LdpcDecoderHip* impl = nullptr;
    // dvbs2_ldpc_decode: device copies of the caller's buffers in `stage` (its stream stays unused), streams and pinned buffers in `pipe`
    dvbs2::HostStage stage; enum { IN, BITS, LLR, RET, N_SLOTS }; static_assert(N_SLOTS <= dvbs2::HostStage::kBufs, "too many staging slots");
    dvbs2::HostPipe pipe;
    int device = 0;
    // experiment / test knobs of the host entries, read ONCE when the handle is created (no getenv per decode call)
    std::string host_plan;      // DVBS2_HOST_PLAN: comma list of chunk sizes, the last one repeats
    int host_chunk = 0;         // DVBS2_HOST_CHUNK: one chunk size for the whole call (0: the measured plan)
    int host_copy_stream = -1;  // DVBS2_HOST_COPY_STREAM: 0 / 1 force the copies off / onto the copy stream (-1: by kind of input buffer)
};

struct dvbs2_bch {
    dvbs2::BchDecoderHip* impl = nullptr;
    dvbs2::HostStage stage; enum { CW, MSG, CORR, N_SLOTS }; static_assert(N_SLOTS <= dvbs2::HostStage::kBufs, "too many staging slots");
    int device = 0;
};

struct dvbs2_demap {
    dvbs2::DemapperHip* impl = nullptr;
    dvbs2::HostStage stage; enum { SYMS, N0, LLR, SNR, N_SLOTS }; static_assert(N_SLOTS <= dvbs2::HostStage::kBufs, "too many staging slots");
    int device = 0;
};
