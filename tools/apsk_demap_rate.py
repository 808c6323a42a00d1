"""HIP-event time per 64 Mi symbols of the stand-alone demapper kernels for notes/apsk_demap.md: 16APSK, 32APSK and 8PSK on normal
frames (about 64 Mi symbols per launch, far more than the last-level cache holds), and a plain device copy that moves the same number
of bytes as each of them (half of 8 + n_mod bytes per symbol read, the same written). Each figure is the median of five regions of four
launches after a warm-up region, scaled to 64 Mi symbols. Prints one JSON line per kernel."""
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


def main():
    import torch
    from dvbs2rx_amd import Demapper, capi
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    base = {}
    for name, constellation, rate in (("8psk", capi.MOD_8PSK, "C3_4"), ("16apsk", capi.MOD_16APSK, "C3_4"), ("32apsk", capi.MOD_32APSK, "C3_4")):
        probe = Demapper(framesize=capi.FECFRAME_NORMAL, rate=rate, constellation=constellation, max_frames=1)
        rows, n_mod = probe.n_syms, probe.n_mod
        probe.close()
        nf = -(-TARGET // rows)
        dm = Demapper(framesize=capi.FECFRAME_NORMAL, rate=rate, constellation=constellation, max_frames=nf)
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
        base[name] = med
        out = dict(kernel=name, frames=nf, rows=rows, bytes_per_symbol=8 + n_mod, regions_ms=[round(m, 4) for m in ms], median_ms_per_64Mi=round(med, 4),
                   algorithmic_TB_per_s=round(TARGET * (8 + n_mod) / med * 1e-9, 3), copy_median_ms_per_64Mi=round(cmed, 4),
                   copy_TB_per_s=round(TARGET * (8 + n_mod) / cmed * 1e-9, 3))
        if name != "8psk":
            out["byte_proportional_ms"] = round(base["8psk"] * (8 + n_mod) / 11.0, 4)
            out["ratio_to_byte_proportional"] = round(med / (base["8psk"] * (8 + n_mod) / 11.0), 3)
        print(json.dumps(out), flush=True)
        dm.close()
        del d_syms, d_llr, src, dst


if __name__ == "__main__":
    main()
