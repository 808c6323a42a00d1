#!/usr/bin/env python3
"""Timings for notes/pulse_shaper.md, to be run on an MI355X: the pulse shaper (symbols -> sps samples per symbol, dvbs2_pulse_shape_device)
at sps 2 and 4 with rrc_delay 5 and at sps 2 with rrc_delay 20, each on 1 stream of 2^26 symbols and on 1024 streams of 2^16, each the
median of five HIP-event regions after one warm-up, next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the same number of bytes as the shaper reads plus writes (dvbs2_rotator_measure's
           copy kernel: 8 bytes in and 8 bytes out per element).
Prints one JSON line per configuration; shaper_of_copy is the shaper's bytes/s over the copy's. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CONFIGS = [(2, 5), (4, 5), (2, 20)]          # (sps, rrc_delay)
BATCHES = [(1, 1 << 26), (1024, 1 << 16)]    # (streams, symbols per stream)


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
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the symbols per stream (a quick look)")
    ap.add_argument("--rolloff", type=float, default=0.2)
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import PulseShaper, capi
    st = torch.cuda.current_stream().cuda_stream
    for sps, delay in CONFIGS:
        for streams, per_stream in BATCHES:
            n = max(1, int(per_stream * a.scale))
            ps = PulseShaper(sps, a.rolloff, delay, max_streams=streams, max_symbols=n)
            d_in = torch.randn((streams * n, 2), dtype=torch.float32, device="cuda")
            d_out = torch.empty((streams * n * sps, 2), dtype=torch.float32, device="cuda")
            t = median_ms(lambda: ps.work_device(d_in.data_ptr(), n, n, streams, d_out.data_ptr(), n * sps, st))
            syms = streams * n
            moved = 8 * syms * (1 + sps)
            r, c = C.c_double(), C.c_double()
            del d_in, d_out  # the copy allocates its own two buffers of moved / 2 bytes each
            torch.cuda.empty_cache()
            capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
            print(json.dumps(dict(sps=sps, rrc_delay=delay, ntaps=ps.ntaps, streams=streams, symbols_per_stream=n, bytes_moved=moved,
                                  shaper_ms=t, shaper_out_samples_per_s=syms * sps / t * 1e3, shaper_GBps=moved / t / 1e6,
                                  copy_ms=c.value, copy_GBps=moved / c.value / 1e6, shaper_of_copy=c.value / t)), flush=True)
            ps.close()


if __name__ == "__main__":
    main()
