#!/usr/bin/env python3
"""Timings for notes/pfbsyn.md, to be run on an MI355X: the polyphase synthesizer (dvbs2_pfbsyn_process_device) on 1 stream with M = 8,
16 and 64 channels, L = M / 2, 16 M + 1 taps and as many input instants as give 2^24 output samples, all channels fed and every fourth,
each the median of five HIP-event regions after one warm-up, next to, in the same run,
  copy     (a) a plain 16-byte-per-lane copy that moves the rows' bytes plus the output bytes once (dvbs2_rotator_measure's copy kernel);
  route    (b) the route the stage replaces: per fed row PulseShaper(L) with the same taps, Rotator(2 pi c / M) in place, and a torch
           += into the wide buffer (cleared first);
  pfbch    (c) PfbChannelizer at the same shape (M, D = L, the same taps, the same selection) on 2^24 input samples: the receive side's
           counterpart of the same bank.
Prints one JSON line per case with output samples per second and the bytes per second against the copy. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CASES = [(M, quarter) for M in (8, 16, 64) for quarter in (False, True)]


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


def lowpass(M, ntaps):
    import numpy as np
    return (np.sinc((np.arange(ntaps) - (ntaps - 1) / 2) / M) * np.hamming(ntaps) / M).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples (a quick look)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvbs2rx_amd import PfbChannelizer, PfbSynthesizer, PulseShaper, Rotator, capi, pfbsyn_tile
    st = torch.cuda.current_stream().cuda_stream
    for M, quarter in CASES:
        Li, ntaps = M // 2, 16 * M + 1
        n_out = max(M, int((1 << 24) * a.scale)) // M * M  # a multiple of M and of L
        n_in = n_out // Li
        taps = lowpass(M, ntaps)
        sel = list(range(0, M, 4)) if quarter else list(range(M))
        d_in = torch.randn((len(sel) * n_in, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty((n_out, 2), dtype=torch.float32, device="cuda")
        sy = PfbSynthesizer(M, Li, taps, max_samples=n_in)
        sy.set_channels(sel)

        def syn_only():
            sy.work_device(d_in.data_ptr(), n_in, n_in, 1, d_out.data_ptr(), n_out, st)  # n_out is a multiple of M: every call does the same work

        t = median_ms(syn_only)
        sy.close()
        moved = 8 * (len(sel) * n_in + n_out)
        row = dict(n_chan=M, interp=Li, ntaps=ntaps, fed=len(sel), instants=n_in, tile=pfbsyn_tile(M, Li, ntaps), out_samples=n_out, bytes_moved=moved,
                   pfbsyn_ms=t, pfbsyn_output_samples_per_s=n_out / t * 1e3, pfbsyn_GBps=moved / t / 1e6, lib=os.path.basename(capi.LIB_PATH))
        # (a) the copy of its bytes
        r, c = C.c_double(), C.c_double()
        capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
        row.update(copy_ms=c.value, copy_GBps=moved / c.value / 1e6, pfbsyn_of_copy=c.value / t)
        # (b) the route it replaces
        shapers = [PulseShaper(Li, taps=taps, max_symbols=n_in) for _ in sel]
        rotators = [Rotator(2.0 * np.pi * chan / M) for chan in sel]
        d_row = torch.empty((n_out, 2), dtype=torch.float32, device="cuda")

        def route():
            d_out.zero_()
            for i in range(len(sel)):
                shapers[i].work_device(d_in.data_ptr() + 8 * i * n_in, n_in, n_in, 1, d_row.data_ptr(), n_out, st)
                rotators[i].work_device(d_row.data_ptr(), n_out, d_row.data_ptr(), st)
                d_out.add_(d_row)

        tr = median_ms(route)
        for o in shapers + rotators:
            o.close()
        row.update(route_ms=tr, route_over_pfbsyn=tr / t)
        del d_row, d_in
        # (c) the channelizer at the same shape
        d_wide = torch.randn((n_out, 2), dtype=torch.float32, device="cuda")
        d_rows = torch.empty((len(sel) * n_in, 2), dtype=torch.float32, device="cuda")
        ch = PfbChannelizer(M, Li, taps, max_samples=n_out)
        ch.set_channels(sel)
        tc = median_ms(lambda: ch.work_device(d_wide.data_ptr(), n_out, n_out, 1, d_rows.data_ptr(), n_in, st))
        ch.close()
        row.update(pfbch_ms=tc, pfbch_over_pfbsyn=tc / t)
        del d_wide, d_rows, d_out
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
