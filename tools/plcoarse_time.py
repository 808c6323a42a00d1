#!/usr/bin/env python3
"""Timings for notes/plcoarse.md, to be run on an MI355X:
  rotator    time per 64 Mi symbols (median of five HIP-event regions) next to a plain 16-byte-per-lane copy of the same bytes
             in the same run (dvbs2_rotator_measure), and their ratio;
  estimator  time per 4096 headers of the two plcoarse kernels together (torch events, median of five) next to
             pl_estimate_kernel's time for the same frames. The split between the two kernels comes from running this script
             under `rocprofv3 --kernel-trace --stats -- python tools/plcoarse_time.py --estimator-only`.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))


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
    ap.add_argument("--symbols", type=int, default=64 << 20)
    ap.add_argument("--headers", type=int, default=4096)
    ap.add_argument("--estimator-only", action="store_true")
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import PlCoarse, PlFrontEnd, capi
    out = {}
    if not a.estimator_only:
        r, c = C.c_double(), C.c_double()
        capi.check(capi.lib.dvbs2_rotator_measure(0, a.symbols, 5, C.byref(r), C.byref(c)))
        gb = a.symbols * 16 / 1e9
        out.update(rotator_symbols=a.symbols, rotator_ms=r.value, copy_ms=c.value, copy_over_rotator=c.value / r.value,
                   rotator_GBps=gb / r.value * 1e3, copy_GBps=gb / c.value * 1e3)
    plsc, n = 4 << 2 | 2 | 1, a.headers  # short QPSK frames with pilots: 8370 symbols each
    fe = PlFrontEnd(0, plsc, max_frames=n)
    L = fe.plframe_len
    st = torch.cuda.current_stream().cuda_stream
    d_x = torch.randn(2 * (n * L + 90), device="cuda")
    d_f = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_c = torch.ones(n, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ph = torch.zeros(n, dtype=torch.float32, device="cuda")
    pc = PlCoarse(1, plsc, max_frames=n)
    out.update(headers=n, plcoarse_ms=median_ms(lambda: pc.work_device(d_x.data_ptr(), L, n, 0, d_f.data_ptr(), 0, d_n.data_ptr(), st)),
               pl_estimate_ms=median_ms(lambda: fe.work_device(d_x.data_ptr(), n, 1, d_c.data_ptr(), 0, 0, st, sof_phase=d_ph.data_ptr())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
