// rotator_hip.h -- the frequency-correcting rotator on the device: rotator_cc::work (reference lib/rotator_cc_impl.cc:36-128).
//   out[n] = in[n] e^{j phi[n]}, phi[n + 1] = phi[n] + inc[n], phi = 0 at the first sample; inc changes at once
//   (set_phase_inc) or at a scheduled ABSOLUTE sample index (schedule), the phase staying continuous. An update whose index
//   is already behind the sample counter when a call reaches it is dropped (:92-95); one beyond the call stays queued.
//   Updates with EQUAL indices are applied in the order they were scheduled, so the last one wins: the reference's
//   priority queue leaves that order open, this is the choice made here.
//
// This is deliberately NOT the reference's arithmetic. gr::rotator keeps a float phasor, multiplies it by e^{j inc} per
// sample and renormalises it every 512 (volk_32fc_s32fc_x2_rotator_32fc): a recurrence along the stream whose error grows
// with the position and which one thread must walk. Here the phase of every sample is evaluated in CLOSED FORM:
//   the phase is kept in turns as unsigned 64-bit fixed point (2^64 = one turn, wrap-around is the modulo); an increment
//   is converted once, in extended precision, to that unit; the stream is cut into segments of constant increment whose
//   start phases are a prefix sum over the update list on the host; sample n of a segment starting at n_s with phase P_s
//   and increment I_s has phase P_s + (n - n_s) I_s in exact integer arithmetic. Its upper 32 bits, as a float in
//   half-turns, go to sincospif, and the product is four float multiplies and two adds (no contraction).
// So any number of threads work on one buffer, the result of a sample does not depend on how the stream is cut into calls
// or on the addresses (in place == out of place, bit for bit), and the error does not grow with the position except
// through the one rounding of an increment: at most (|inc| / 2 pi) 2^-63 + 2^-65 turns per sample of its segment.
// VOLK is not available to pin the recurrence against, so the output is tested against a float64 evaluation of the exact
// phase under a derived bound (tests/plcoarse_model.py) and is UNPINNED against the genuine reference.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "device_stage.h"

namespace dvbs2 {

// median over `regions` HIP-event regions of one rotation of n_syms symbols (one segment, out of place) and, in the same run, of a
// plain 16-byte-per-lane copy of the same bytes on the same grid; 0, or the StageCode of the failure with its text in *err
int rotator_measure(int device, int n_syms, int regions, double* rot_ms, double* copy_ms, std::string* err);

class RotatorHip : public DeviceStage {
public:
    RotatorHip(double phase_inc, int device);
    void reset(); // the handle as constructed: counter 0, phase 0, the constructor's increment, empty queue
    int set_phase_inc(double inc);
    int schedule(int64_t offset, double inc);
    int64_t position() const { return counter_; }
    int queued() const { return (int)queue_.size(); }
    uint64_t phase() const { return phase_; }
    // advances counter and phase over n samples as a call would, applying and dropping updates, without touching data
    int seek(int64_t n);
    // DEVICE pointers, 8-byte aligned; d_out == d_in is allowed, any other overlap is not. Asynchronous on `stream`
    int rotate_device(const float* d_in, int n_syms, float* d_out, hipStream_t stream);

private:
    struct Update { int64_t offset; double inc; };
    struct Segment { int64_t start; uint64_t phase, inc; }; // start relative to the call
    void advance(int64_t n, std::vector<Segment>* segs);
    double inc0_;
    int64_t counter_ = 0;
    uint64_t phase_ = 0, inc_ = 0;
    std::vector<Update> queue_; // ascending offset, equal offsets in scheduling order
};

} // namespace dvbs2
