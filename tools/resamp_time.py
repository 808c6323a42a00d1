#!/usr/bin/env python3
"""Timings for notes/resampler.md, to be run on an MI355X: the resampler (dvbs2_resamp_process_device) at rate 2.5 and at 1 + 1e-4 with 32
branches of the transmit prototype (D = 5: 321 taps, L = 11 terms per bank), each on 1 stream of 2^24 samples and on 1024 streams of 2^14,
each the median of five HIP-event regions after one warm-up, next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the same number of bytes as the resampler reads plus writes (dvbs2_rotator_measure's
           copy kernel: 8 bytes in and 8 bytes out per element);
  shaper   dvbs2_pulse_shape_device at sps 2 writing the same number of output samples, with the rrc_delay that gives as many terms per
           output sample as this stage runs through its two banks (2 L = 22: rrc_delay 11 has 23 and 22).
Prints one JSON line per configuration; resamp_of_copy is the resampler's bytes/s over the copy's, resamp_of_shaper its output samples/s over
the shaper's. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

RATES = [2.5, 1 + 1e-4]
BATCHES = [(1, 1 << 24), (1024, 1 << 14)]  # (streams, input samples per stream)
NFILTS, ROLLOFF, D = 32, 0.2, 5


def median_ms(fn, regions=5):
    import torch
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return sorted(t)[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples per stream (a quick look)")
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import PulseShaper, Resampler, capi, pulse_taps
    st = torch.cuda.current_stream().cuda_stream
    taps = pulse_taps(NFILTS, ROLLOFF, D, 0.0, NFILTS)
    for rate in RATES:
        for streams, per_stream in BATCHES:
            n = max(1, int(per_stream * a.scale))
            rs = Resampler(NFILTS, taps, rate, max_streams=streams, max_samples=n)
            stride = int(rs.produce(n, streams).max()) + 1
            d_in = torch.randn((streams * n, 2), dtype=torch.float32, device="cuda")
            d_out = torch.empty((streams * stride, 2), dtype=torch.float32, device="cuda")
            outs = []

            def call():
                outs.append(int(rs.work_device(d_in.data_ptr(), n, n, streams, d_out.data_ptr(), stride, st).sum()))
            t = median_ms(call)
            n_out = outs[-1]  # (within one sample per stream of every other call's)
            moved = 8 * (streams * n + n_out)
            terms = 2 * rs.terms
            rs.close()
            del d_in, d_out
            torch.cuda.empty_cache()
            # the shaper at sps 2 on n_out / 2 symbols, spread over the same streams
            delay = terms // 2
            syms = max(1, n_out // 2 // streams)
            ps = PulseShaper(2, ROLLOFF, delay, max_streams=streams, max_symbols=syms)
            p_in = torch.randn((streams * syms, 2), dtype=torch.float32, device="cuda")
            p_out = torch.empty((streams * syms * 2, 2), dtype=torch.float32, device="cuda")
            tp = median_ms(lambda: ps.work_device(p_in.data_ptr(), syms, syms, streams, p_out.data_ptr(), syms * 2, st))
            ps.close()
            del p_in, p_out  # the copy allocates its own two buffers of moved / 2 bytes each
            torch.cuda.empty_cache()
            r, c = C.c_double(), C.c_double()
            capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
            print(json.dumps(dict(rate=rate, nfilts=NFILTS, ntaps=int(taps.size), terms_per_output=terms, streams=streams, samples_per_stream=n,
                                  out_samples=n_out, bytes_moved=moved, resamp_ms=t, resamp_out_samples_per_s=n_out / t * 1e3,
                                  resamp_GBps=moved / t / 1e6, copy_ms=c.value, copy_GBps=moved / c.value / 1e6, resamp_of_copy=c.value / t,
                                  shaper_rrc_delay=delay, shaper_out_samples=streams * syms * 2, shaper_ms=tp,
                                  shaper_out_samples_per_s=streams * syms * 2 / tp * 1e3,
                                  resamp_of_shaper=(n_out / t) / (streams * syms * 2 / tp))), flush=True)


if __name__ == "__main__":
    main()
