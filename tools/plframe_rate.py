#!/usr/bin/env python3
"""HIP-event time of dvbs2_plframe_process_device (estimates + payload step from whole PLFRAMEs) for resident frames, against
dvbs2_plpayload_process_device on the same payloads with precomputed parameters, in the same run: five regions of K calls
each, median. Prints one table row per geometry (notes/plframe_front_end.md)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))
from dvbs2rx_amd import PlFrontEnd, PlPayload, capi  # noqa: E402

CASES = [("8PSK 3/4 normal, pilots", (14 << 2) | 1), ("QPSK 1/2 short, pilots", (4 << 2) | 3), ("QPSK 1/2 normal, pilotless", 4 << 2)]


def timed(fn, k, regions=5):
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / k)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--gold", type=int, default=5)
    args = ap.parse_args()
    nf, st = args.frames, torch.cuda.current_stream().cuda_stream
    print("| geometry | plframe_len | payload step alone (ms) | estimates alone (ms) | front end (ms) | front end / payload step | Msym/s |")
    print("|---|---|---|---|---|---|---|")
    for name, plsc in CASES:
        fe = PlFrontEnd(args.gold, plsc, max_frames=nf)
        pp = PlPayload(args.gold, fe.n_slots, fe.n_pilots > 0, max_frames=nf)
        gen = torch.Generator(device="cuda").manual_seed(plsc)
        x = torch.randn((nf * fe.plframe_len + 90, 2), generator=gen, device="cuda", dtype=torch.float32) * 0.7071
        cc = torch.ones(nf, dtype=torch.int32, device="cuda")
        cf = torch.zeros(nf, dtype=torch.float32, device="cuda")
        out = torch.empty((nf, fe.xfecframe_len, 2), dtype=torch.float32, device="cuda")
        out2 = torch.empty_like(out)
        hph, fine = torch.zeros(nf, device="cuda"), torch.zeros(nf, device="cuda")
        pil = torch.zeros((nf, max(fe.n_pilots, 1)), device="cuda")
        fe.work_device(x.data_ptr(), nf, 1, cc.data_ptr(), cf.data_ptr(), out.data_ptr(), st, plheader_phase=hph.data_ptr(),
                       fine_foffset=fine.data_ptr(), pilot_phase=pil.data_ptr() if fe.n_pilots else 0)
        inc = (2.0 * np.pi * fine.double()).float()
        pay = x[:nf * fe.plframe_len].reshape(nf, fe.plframe_len, 2)[:, 90:].contiguous()  # the payload slices back to back

        def base():
            capi.check(capi.lib.dvbs2_plpayload_process_device(pp._h, pay.data_ptr(), nf, hph.data_ptr(), inc.data_ptr(), cc.data_ptr(),
                                                               pil.data_ptr(), out2.data_ptr(), st))

        def front():
            fe.work_device(x.data_ptr(), nf, 1, cc.data_ptr(), cf.data_ptr(), out.data_ptr(), st)

        def est_only():
            fe.work_device(x.data_ptr(), nf, 1, cc.data_ptr(), cf.data_ptr(), 0, st, fine_foffset=fine.data_ptr())

        base()
        torch.cuda.synchronize()
        assert torch.equal(out, out2), "front end and payload step disagree"
        for f in (base, front, est_only):
            timed(f, 3, 1)
        tb, tf, te = timed(base, args.calls), timed(front, args.calls), timed(est_only, args.calls)
        print(f"| {name} | {fe.plframe_len} | {tb:.4f} | {te:.4f} | {tf:.4f} | {tf / tb:.3f} | {nf * fe.plframe_len / tf / 1e3:.0f} |", flush=True)
        fe.close()
        pp.close()


if __name__ == "__main__":
    main()
