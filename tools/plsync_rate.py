#!/usr/bin/env python3
"""Rates of the PLFRAME search (dvbs2_plsync_*) on resident buffers, HIP-event times, median of five regions
(notes/plsync.md):
  1. the metric kernel in symbols/s and bytes/s (8 B in + 4 B out per symbol) against a hand-written 16-byte device-to-device
     copy moving the same 12 B per symbol, in the same run (tools/plsync_rate_copy.hip);
  2. the tracker (search minus metric): microseconds per locked frame on a clean CCM stream, per 1 M symbols on a stream
     without headers (searching throughout), and on a stream with frequent false crossings (0 dB, decoding at each);
  3. a plain-C RESTATEMENT of the reference's per-symbol loop on one CPU core (tools/plsync_rate_cpu.c; not the reference).
The two helpers are compiled into tools/bin/ on first use (--build-only: just that)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build():
    os.makedirs(BIN, exist_ok=True)
    jobs = [(os.path.join(ROOT, "tools", "plsync_rate_copy.hip"), os.path.join(BIN, "libplsync_rate_copy.so"),
             [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC", "-shared"]),
            (os.path.join(ROOT, "tools", "plsync_rate_cpu.c"), os.path.join(BIN, "libplsync_rate_cpu.so"),
             [os.environ.get("CC", "cc"), "-O2", "-fPIC", "-shared", "-std=c99"])]
    for src, out, cmd in jobs:
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            subprocess.check_call(cmd + [src, "-o", out, "-lm"] if src.endswith(".c") else cmd + [src, "-o", out])
    return jobs[0][1], jobs[1][1]


def timed(fn, k, regions=5, before=None):
    import torch
    ms = []
    for _ in range(regions):
        if before:
            before()
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
    ap.add_argument("--symbols", type=int, default=64 << 20, help="resident buffer of the metric / copy comparison")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cpu-symbols", type=int, default=4 << 20)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    copy_so, cpu_so = build()
    if args.build_only:
        return
    import torch
    import plframe_model as M
    import plsync_model as P
    from dvbs2rx_amd import PlSync, plsync_taps
    st = torch.cuda.current_stream().cuda_stream

    # ---- 1. metric kernel against the copy
    n = args.symbols
    cp = C.CDLL(copy_so)
    cp.plsync_rate_copy16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    x = torch.randn((n, 2), device="cuda", dtype=torch.float32) * 0.7071
    met = torch.empty(n, device="cuda", dtype=torch.float32)
    n16 = n * 6 // 16  # 6 B per symbol read and 6 B written: 12 B per symbol in all, as the metric kernel's 8 + 4
    src, dst = torch.empty(n16 * 4, device="cuda"), torch.empty(n16 * 4, device="cuda")
    src.normal_()
    ps = PlSync(max_symbols=n, max_frames=16)

    def run_metric():
        ps.metric_device(x.data_ptr(), n, met.data_ptr(), st)

    def run_copy():
        assert cp.plsync_rate_copy16(dst.data_ptr(), src.data_ptr(), n16, st) == 0

    for f in (run_metric, run_copy):
        timed(f, 2, 1)
    assert torch.equal(src, dst)
    tm, tc = timed(run_metric, args.calls), timed(run_copy, args.calls)
    print(f"metric kernel: {n} symbols in {tm:.3f} ms = {n / tm / 1e6:.1f} Gsym/s, {12 * n / tm / 1e9:.2f} TB/s of 8 B in + 4 B out")
    print(f"16-byte copy of the same 12 B per symbol: {tc:.3f} ms = {n / tc / 1e6:.1f} Gsym/s equivalent, {32 * n16 / tc / 1e9:.2f} TB/s")
    print(f"metric / copy time: {tm / tc:.2f}")
    ps.close()
    del x, met, src, dst

    # ---- 2. tracker cost
    rng = np.random.default_rng(1)
    plsc = P.SHORT_QPSK
    L = M.pls_parse(plsc)["plframe_len"]
    frame = M.make_plframes(plsc, 0, 1, rng)[0].reshape(-1)
    nfr = 2000
    locked_stream = np.concatenate([P.qpsk(rng, 1000).astype(np.complex64), np.tile(frame, nfr), frame[:90], P.qpsk(rng, 300)]).astype(np.complex64)
    junk = (P.qpsk(rng, 16 << 20) * 0.5).astype(np.complex64)  # a quarter of unit power: the metric never reaches 30
    noisy, _, _ = P.make_stream([plsc] * 500, 7, es_n0_db=0.0, offset=1000)
    assert locked_stream.dtype == junk.dtype == noisy.dtype == np.complex64
    for what, xs, per in (("clean CCM stream, locked", locked_stream, "frame"), ("no headers, searching throughout", junk, "msym"),
                          ("0 dB stream, a decode at every crossing", noisy, "msym")):
        d_x = torch.from_numpy(xs.view(np.float32)).cuda()
        ps = PlSync(max_symbols=xs.size, max_frames=1 << 17)
        d_f = torch.zeros((1 << 17) * 16, dtype=torch.uint8, device="cuda")
        d_m = torch.empty(xs.size, device="cuda", dtype=torch.float32)
        t_all = timed(lambda: ps.work_device(d_x.data_ptr(), xs.size, d_f.data_ptr(), st), 1, 5, before=ps.reset)
        nf, consumed, state = ps.finish()
        t_met = timed(lambda: ps.metric_device(d_x.data_ptr(), xs.size, d_m.data_ptr(), st), 1, 5)
        t_trk = (t_all - t_met) * 1e3
        unit = f"{t_trk / max(nf, 1):.3f} us per frame record" if per == "frame" else f"{t_trk / (xs.size / 1e6):.1f} us per 1 M symbols"
        print(f"tracker, {what}: {xs.size} symbols, {nf} records, final state {state}; search {t_all:.3f} ms, metric alone {t_met:.3f} ms, "
              f"tracker {t_trk:.0f} us = {unit}; the metric of a call of {xs.size} symbols takes {t_met / t_all * 100:.0f} % of it")
        ps.close()

    # ---- 3. the plain-C restatement on one core
    cpu = C.CDLL(cpu_so)
    cpu.plsync_rate_cpu.restype = C.c_int64
    cpu.plsync_rate_cpu.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    sof, pl = plsync_taps()
    sof_rev, pl_rev = np.ascontiguousarray(sof[::-1]), np.ascontiguousarray(pl[::-1])  # newest differential first
    for what, xs in (("searching throughout", junk[:args.cpu_symbols]), ("locked", locked_stream[:args.cpu_symbols])):
        xs = np.ascontiguousarray(xs)
        lk = C.c_int()
        t0 = time.perf_counter()
        h = cpu.plsync_rate_cpu(xs.ctypes.data, xs.size, sof_rev.ctypes.data, pl_rev.ctypes.data, L, 3, C.byref(lk))
        dt = time.perf_counter() - t0
        print(f"plain-C restatement (NOT the reference), one core, {what}: {xs.size} symbols in {dt * 1e3:.1f} ms = "
              f"{xs.size / dt / 1e6:.1f} Msym/s, {h} headers, locked {lk.value}")


if __name__ == "__main__":
    main()
