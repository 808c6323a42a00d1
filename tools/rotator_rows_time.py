#!/usr/bin/env python3
"""Times of the rotator rows against the route they replace and against a copy of their bytes (notes/rotator_rows.md): HIP-event times on
resident buffers, medians over --regions regions, out of place.
  rows      rotator_rows_device: S rows of n samples in ONE launch from records in device memory;
  replaced  S single Rotator handles called one after the other on one stream (S launches). With --parent-lib PATH the handles come
            from THAT library -- libdvbs2_fec_hip.so built from the parent commit, loaded next to the product library in the same
            process -- so that the yardstick is not the code under test; without it they are the product library's own;
  copy      dvbs2_rotator_measure's 16-byte-per-lane copy kernel over the same S * n samples (it also gives the product library's
            single handle over all of them as one stream, in the same run).
S * n = 2^24 samples for S in 1, 8, 64, 1024. Then the control step for 1024 streams with 16 slots each next to the smallest launch
the section has (one retune: a single lane). Prints markdown table rows."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))


def timed(fn, regions):
    import torch
    ms = []
    for r in range(-1, regions):  # region -1 warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= 0:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.max(ms) - np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=24, help="S * n = 2^this samples")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 64, 1024])
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--parent-lib", default=os.environ.get("DVBS2_PARENT_LIB"), help="libdvbs2_fec_hip.so of the parent commit: the replaced route")
    args = ap.parse_args()
    import torch
    from dvbs2rx_amd import capi, rotator_control_device, rotator_retune_device, rotator_rows_device, rotator_state_init
    st = torch.cuda.current_stream().cuda_stream
    total = 1 << args.log2_samples
    old = capi.lib
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("dvbs2_rotator_create", "dvbs2_rotator_destroy", "dvbs2_rotator_rotate_device"):
            getattr(old, name).restype, getattr(old, name).argtypes = capi.SYMBOLS[name]
        assert not hasattr(old, "dvbs2_rotator_rows_device"), "--parent-lib already has the rotator rows: it is not the parent's library"
    print(f"replaced route from {'the parent library ' + args.parent_lib if args.parent_lib else 'the product library itself'}")
    rot_ms, copy_ms = C.c_double(), C.c_double()
    capi.check(capi.lib.dvbs2_rotator_measure(0, total, args.regions, C.byref(rot_ms), C.byref(copy_ms)))
    print(f"dvbs2_rotator_measure over 2^{args.log2_samples} samples: single handle {rot_ms.value:.4f} ms, copy {copy_ms.value:.4f} ms "
          f"({2 * 8 * total / copy_ms.value * 1e-6:.0f} GB/s read + written)")
    d_in = torch.randn((total, 2), device="cuda", dtype=torch.float32)
    d_out = torch.empty_like(d_in)
    print("| rows S | samples per row | rows, ms | spread | replaced (S handles), ms | spread | copy, ms | rows / copy | replaced / rows |")
    print("| --- | --- | --- | --- | --- | --- | --- | --- | --- |")
    for S in args.streams:
        n = total // S
        incs = [0.001 * (s + 1) for s in range(S)]
        d_state = torch.from_numpy(rotator_state_init(incs).view(np.uint8)).cuda()
        handles = []
        for inc in incs:
            h = C.c_void_p()
            capi.check(old.dvbs2_rotator_create(C.byref(h), inc, 0))
            handles.append(h)

        def rows():
            rotator_rows_device(d_in.data_ptr(), n, d_out.data_ptr(), n, n, S, 0, d_state.data_ptr(), 0, st)

        def replaced():
            for s, h in enumerate(handles):
                old.dvbs2_rotator_rotate_device(h, d_in.data_ptr() + 8 * n * s, n, d_out.data_ptr() + 8 * n * s, st)

        # the first region of each handle is sample 0: the two routes must give the same bits
        rows()
        torch.cuda.synchronize()
        want = d_out.clone()
        replaced()
        torch.cuda.synchronize()
        assert torch.equal(want.view(torch.int32), d_out.view(torch.int32)), "the two routes differ"
        t_rows, sp_rows = timed(rows, args.regions)
        t_rep, sp_rep = timed(replaced, args.regions)
        print(f"| {S} | {n} | {t_rows:.4f} | {sp_rows:.4f} | {t_rep:.4f} | {sp_rep:.4f} | {copy_ms.value:.4f} | {t_rows / copy_ms.value:.3f} | "
              f"{t_rep / t_rows:.2f} |", flush=True)
        for h in handles:
            old.dvbs2_rotator_destroy(h)
    S, per = 1024, 16
    d_state = torch.from_numpy(rotator_state_init([0.0] * S).view(np.uint8)).cuda()
    d_off = torch.arange(0, (S + 1) * per, per, dtype=torch.int32, device="cuda")
    d_f = torch.full((S * per,), 1e-4, dtype=torch.float32, device="cuda")
    d_one = torch.ones(S * per, dtype=torch.int32, device="cuda")
    d_applied, d_delta = torch.zeros(S, dtype=torch.int32, device="cuda"), torch.zeros(S, dtype=torch.int64, device="cuda")
    t_ctl, sp_ctl = timed(lambda: rotator_control_device(d_off.data_ptr(), S, S * per, d_f.data_ptr(), d_one.data_ptr(), d_one.data_ptr(), d_f.data_ptr(),
                                                         d_one.data_ptr(), 0.5, 0.5, 1 << 20, d_state.data_ptr(), d_applied.data_ptr(), d_delta.data_ptr(),
                                                         0, st), args.regions)
    t_one, sp_one = timed(lambda: rotator_retune_device(d_state.data_ptr(), 0, 1 << 20, 0.1, 0, st), args.regions)
    torch.cuda.synchronize()
    assert d_applied.cpu().tolist() == [2] * S
    print(f"control step, {S} streams of {per} slots: {t_ctl * 1e3:.1f} us (spread {sp_ctl * 1e3:.1f}); one retune, a single lane: {t_one * 1e3:.1f} us "
          f"(spread {sp_one * 1e3:.1f})")


if __name__ == "__main__":
    main()
