#!/usr/bin/env python3
"""Timings for notes/agc.md, to be run on an MI355X: the AGC (dvbs2_agc_work_device) on 1 stream of 2^22 samples, 64 streams of 2^20 and
4096 streams of 2^16, each out of place without and with the gain output and in place, each the median of five HIP-event regions after
one warm-up, next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the same number of bytes as the AGC reads plus writes (dvbs2_rotator_measure's copy
           kernel: 8 bytes in and 8 bytes out per element).
Prints one JSON line per point; agc_of_copy is the AGC's bytes/s over the copy's. The recurrence is serial in time, so a point's rate is
streams times the rate of one dependent chain until the batch fills the device. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

BATCHES = [(1, 1 << 22), (64, 1 << 20), (4096, 1 << 16)]  # (streams, samples per stream)
MODES = ["out_of_place", "with_gain", "in_place"]


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
    ap.add_argument("--rate", type=float, default=1e-5)
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import Agc, capi
    st = torch.cuda.current_stream().cuda_stream
    for streams, per_stream in BATCHES:
        n = max(1, int(per_stream * a.scale))
        agc = Agc(a.rate, 1.0, 1.0, 65536.0, max_streams=streams, max_samples=n)
        d_in = torch.randn((streams * n, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty_like(d_in)
        d_gain = torch.empty(streams * n, dtype=torch.float32, device="cuda")
        calls = dict(out_of_place=lambda: agc.work_device(d_in.data_ptr(), n, n, streams, d_out.data_ptr(), n, 0, 0, st),
                     with_gain=lambda: agc.work_device(d_in.data_ptr(), n, n, streams, d_out.data_ptr(), n, d_gain.data_ptr(), n, st),
                     in_place=lambda: agc.work_device(d_out.data_ptr(), n, n, streams, d_out.data_ptr(), n, 0, 0, st))
        times = {m: median_ms(calls[m]) for m in MODES}
        agc.close()
        del d_in, d_out, d_gain  # the copy allocates its own two buffers
        torch.cuda.empty_cache()
        samples = streams * n
        for m in MODES:
            moved = samples * (20 if m == "with_gain" else 16)
            r, c = C.c_double(), C.c_double()
            capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
            t = times[m]
            print(json.dumps(dict(mode=m, streams=streams, samples_per_stream=n, tile=capi.AGC_TILE, bytes_moved=moved, agc_ms=t,
                                  agc_samples_per_s=samples / t * 1e3, agc_samples_per_s_per_stream=n / t * 1e3, agc_GBps=moved / t / 1e6,
                                  copy_ms=c.value, copy_GBps=moved / c.value / 1e6, agc_of_copy=c.value / t)), flush=True)


if __name__ == "__main__":
    main()
