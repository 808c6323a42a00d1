#!/usr/bin/env python3
"""Timings for notes/plframer.md, to be run on an MI355X: output symbols/s of the PL framer (XFECFRAMEs -> PLFRAMEs, one launch) for
QPSK normal with pilots x 4096 frames and short QPSK without pilots x 16384, each the median of five event regions after one warm-up,
next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the same number of bytes as the framer reads plus writes (dvbs2_rotator_measure's
           copy kernel: 8 bytes in and 8 bytes out per element).
Prints one JSON line per configuration; framer_of_copy is the framer's bytes/s over the copy's. The sequence is CCM (every frame the
same PLSC) with a closing header."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CONFIGS = [("qpsk_normal_pilots", (4 << 2) | 1, 4096), ("qpsk_short_nopilots", (4 << 2) | 2, 16384)]


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
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the frame counts (a quick look)")
    ap.add_argument("--gold", type=int, default=0)
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import PlFramer, capi
    st = torch.cuda.current_stream().cuda_stream
    for name, plsc, frames in CONFIGS:
        nf = max(1, int(frames * a.scale))
        fr = PlFramer(a.gold, max_frames=nf)
        fr.set_sequence([plsc] * nf)
        d_in = torch.randn((fr.in_syms, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty((fr.out_syms + 90, 2), dtype=torch.float32, device="cuda")
        t = median_ms(lambda: fr.work_device(d_in.data_ptr(), nf, plsc, d_out.data_ptr(), st))
        moved = 8 * (fr.in_syms + fr.out_syms + 90)
        r, c = C.c_double(), C.c_double()
        del d_in, d_out  # the copy allocates its own two buffers of moved / 2 bytes each
        torch.cuda.empty_cache()
        capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
        print(json.dumps(dict(config=name, plsc=plsc, frames=nf, in_syms=fr.in_syms, out_syms=fr.out_syms + 90, bytes_moved=moved,
                              framer_ms=t, framer_out_syms_per_s=(fr.out_syms + 90) / t * 1e3, framer_GBps=moved / t / 1e6,
                              copy_ms=c.value, copy_out_syms_per_s=(fr.out_syms + 90) / c.value * 1e3, copy_GBps=moved / c.value / 1e6,
                              framer_of_copy=c.value / t)), flush=True)
        fr.close()


if __name__ == "__main__":
    main()
