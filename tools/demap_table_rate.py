"""HIP-event time per 64 Mi symbols of the caller-table demapper kernel for notes/demap_table.md, on normal frames (about 64 Mi symbols
per launch, far more than the last-level cache holds): the table kernel at 8, 16, 32, 64 and 256 points, the built-in 16APSK and
32APSK kernels on the same symbols as the 16- and 32-point arms, the 8PSK kernel (the base of the byte-proportional time) and a plain
device copy that moves the same number of bytes as each arm (half of 8 + n_mod bytes per symbol read, the same written). Each figure
is the median of five regions of four launches after a warm-up region, scaled to 64 Mi symbols; every region is listed. Prints one
JSON line per arm.

--arms table | builtin | all. The built-in arms are the yardstick of the 16- and 32-point table arms and belong to the library of
the commit before this kernel: run them with DVBS2_LIB pointing at that build (capi.py) and --arms builtin."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

TARGET = 64 << 20
LAUNCHES = 4


def regions(fn):
    import torch
    ms = []
    for region in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        torch.cuda.synchronize()
        if region:
            ms.append(a.elapsed_time(b) / LAUNCHES)
    return ms


def ring_table(sizes, radii, seed):
    """rings of sizes[k] points at radii[k], Es = 1, labels a seeded permutation (the time does not depend on the labelling)"""
    p = np.concatenate([r * np.exp(2j * np.pi * (np.arange(n) + 0.5 * (k % 2 == 0)) / n) for k, (n, r) in enumerate(zip(sizes, radii))])
    p = p / np.sqrt(np.mean(np.abs(p) ** 2))
    return p[np.random.default_rng(seed).permutation(len(p))].astype(np.complex64)


def main():
    import torch
    from dvbs2rx_amd import Demapper, apsk_points, capi
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", choices=("table", "builtin", "all"), default="all")
    args = ap.parse_args()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    builtin = [("8psk", lambda mf: Demapper(framesize=capi.FECFRAME_NORMAL, rate="C3_4", constellation=capi.MOD_8PSK, max_frames=mf)),
               ("16apsk", lambda mf: Demapper(framesize=capi.FECFRAME_NORMAL, rate="C3_4", constellation=capi.MOD_16APSK, max_frames=mf)),
               ("32apsk", lambda mf: Demapper(framesize=capi.FECFRAME_NORMAL, rate="C3_4", constellation=capi.MOD_32APSK, max_frames=mf))]
    table = []
    if args.arms != "builtin":
        tables = [("table8", ring_table((1, 7), (0.0, 1.0), 8)), ("table16", apsk_points(capi.MOD_16APSK, "C3_4")),
                  ("table32", apsk_points(capi.MOD_32APSK, "C3_4")), ("table64", ring_table((4, 12, 20, 28), (1.0, 2.2, 3.4, 4.6), 64)),
                  ("table256", ring_table((32,) * 8, tuple(1.0 + 0.75 * k for k in range(8)), 256))]
        # 16 points in natural order would be routed to the built-in kernel: that arm takes the reversed column order to stay on the table kernel
        table = [(name, (lambda mf, p=p: Demapper.from_table(capi.FECFRAME_NORMAL, p, (3, 2, 1, 0) if len(p) == 16 else None, max_frames=mf)))
                 for name, p in tables]
    arms = builtin[:1] + (builtin[1:] if args.arms != "table" else []) + table
    base = None
    for name, make in arms:
        probe = make(1)
        rows, n_mod = probe.n_syms, probe.n_mod
        probe.close()
        nf = -(-TARGET // rows)
        dm = make(nf)
        one = (rng.normal(size=(64, rows)) + 1j * rng.normal(size=(64, rows))).astype(np.complex64)  # symbols all over the plane
        d_syms = torch.from_numpy(one.view(np.float32)).cuda().repeat(-(-nf // 64), 1)[:nf].contiguous()
        d_n0 = torch.full((1,), 0.05, dtype=torch.float32, device="cuda")
        d_llr = torch.zeros((nf, rows * n_mod), dtype=torch.int8, device="cuda")
        scale = TARGET / (nf * rows)
        ms = [m * scale for m in regions(lambda: dm.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_llr.data_ptr(), st))]
        half = nf * rows * (8 + n_mod) // 2
        src = torch.zeros(half, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        cp = [m * scale for m in regions(lambda: dst.copy_(src))]
        med, cmed = float(np.median(ms)), float(np.median(cp))
        if name == "8psk":
            base = med
        out = dict(kernel=name, lib=os.path.basename(capi.LIB_PATH), frames=nf, rows=rows, bytes_per_symbol=8 + n_mod, regions_ms=[round(m, 4) for m in ms],
                   median_ms_per_64Mi=round(med, 4), algorithmic_TB_per_s=round(TARGET * (8 + n_mod) / med * 1e-9, 3),
                   copy_regions_ms=[round(m, 4) for m in cp], copy_median_ms_per_64Mi=round(cmed, 4), copy_TB_per_s=round(TARGET * (8 + n_mod) / cmed * 1e-9, 3))
        if name != "8psk":
            out["byte_proportional_ms"] = round(base * (8 + n_mod) / 11.0, 4)
            out["ratio_to_byte_proportional"] = round(med / (base * (8 + n_mod) / 11.0), 3)
        print(json.dumps(out), flush=True)
        dm.close()
        del d_syms, d_llr, src, dst


if __name__ == "__main__":
    main()
