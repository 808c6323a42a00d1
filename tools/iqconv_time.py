#!/usr/bin/env python3
"""Timings for notes/iqconv.md, to be run on an MI355X: the IQ sample converter (dvbs2_iqconv_unpack_device / _pack_device) for u8 and
s16 on 1 row of 2^26 samples and on 4096 rows of 32400, with and without statistics, each the median of HIP-event regions after one
warm-up, next to, on the same buffers in the same run,
  copy     a plain device-to-device copy of the same total bytes (in + out of the stage: a copy of half of them reads and writes that),
  torch    the expression the stage replaces on the device: codes.to(float32), subtract, multiply -- and multiply, add, round, clamp,
           to(dtype) the other way --, a kernel and a pass over the floats per operation,
and, for u8 on the one-row shape, the host link: dvbs2_iqconv_unpack_to_device of n samples of codes from a dvbs2_host_alloc buffer
against a host-to-device copy of n float32 pairs from the same kind of buffer (what crosses the link when the CPU converts).
Prints one JSON line per format, shape and direction. Asserts nothing."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

SHAPES = [(1, 1 << 26), (4096, 32400)]  # (rows, samples per row)


def median_ms(fn, regions):
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


def median_host_ms(fn, regions):
    """for the synchronous host entries: a host clock around a call that returns with the device idle"""
    import torch
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(regions):
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - a) * 1e3)
    return sorted(t)[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples per row (a quick look)")
    ap.add_argument("--regions", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvbs2rx_amd import HostBuffer, IqConverter, capi
    st = torch.cuda.current_stream().cuda_stream
    for fmt, dtype, full, bias, lo, hi in (("u8", torch.uint8, 128.0, 127.5, 0, 255), ("s16", torch.int16, 32768.0, 0.0, -32768, 32767)):
        for rows, per_row in SHAPES:
            n = max(1, int(per_row * a.scale))
            conv = IqConverter(fmt, 1.0, max_streams=rows, max_samples=n)
            d_codes = torch.randint(lo, hi + 1, (rows, n, 2), dtype=dtype, device="cuda")
            d_floats = torch.empty((rows, n, 2), dtype=torch.float32, device="cuda")
            d_stats = torch.zeros((rows, 3), dtype=torch.int64, device="cuda")
            total = d_codes.numel() * d_codes.element_size() + 4 * d_floats.numel()
            d_a = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
            d_b = torch.empty_like(d_a)
            c, f, s = d_codes.data_ptr(), d_floats.data_ptr(), d_stats.data_ptr()

            def torch_unpack():
                x = d_codes.to(torch.float32)
                if bias:
                    x -= bias
                x *= 1.0 / full
                return x

            def torch_pack():
                x = d_floats * full
                if bias:
                    x += bias
                return x.round_().clamp_(lo, hi).to(dtype)

            calls = dict(unpack=dict(stage=lambda: conv.unpack_device(c, n, n, rows, f, n, 0, st),
                                     stage_stats=lambda: conv.unpack_device(c, n, n, rows, f, n, s, st), torch=torch_unpack),
                         pack=dict(stage=lambda: conv.pack_device(f, n, n, rows, c, n, 0, st),
                                   stage_stats=lambda: conv.pack_device(f, n, n, rows, c, n, s, st), torch=torch_pack))
            conv.unpack_device(c, n, n, rows, f, n, 0, st)  # floats inside full scale for the pack that follows
            for direction, fns in calls.items():
                ms = {k: median_ms(fn, a.regions) for k, fn in fns.items()}
                ms["copy"] = median_ms(lambda: d_b.copy_(d_a), a.regions)
                out = dict(format=fmt, direction=direction, rows=rows, samples_per_row=n, tile=capi.IQCONV_TILE, bytes_in_plus_out=total)
                out.update({k + "_ms": round(v, 4) for k, v in ms.items()})
                out.update(stage_GBps=round(total / ms["stage"] / 1e6, 1), stage_stats_GBps=round(total / ms["stage_stats"] / 1e6, 1),
                           copy_GBps=round(total / ms["copy"] / 1e6, 1), stage_of_copy=round(ms["copy"] / ms["stage"], 3),
                           stage_stats_of_copy=round(ms["copy"] / ms["stage_stats"], 3), stage_of_torch=round(ms["torch"] / ms["stage"], 2))
                print(json.dumps(out), flush=True)
            if fmt == "u8" and rows == 1:
                host_codes = HostBuffer((n, 2), np.uint8)
                host_floats = HostBuffer((n, 2), np.float32)
                host_codes.array[:] = 128
                host_floats.array[:] = 0.25
                words = np.zeros(3, np.uint64)
                t_floats = torch.from_numpy(host_floats.array)  # page-locked: the copy is one DMA at the link's rate
                link = dict(unpack_to_device=lambda: conv.unpack_to_device(host_codes.array, f),
                            unpack_to_device_stats=lambda: capi.lib.dvbs2_iqconv_unpack_to_device(conv._h, host_codes.ptr, n, f, words.ctypes.data),
                            floats_h2d=lambda: d_floats[0].copy_(t_floats, non_blocking=True))
                ms = {k: median_host_ms(fn, a.regions) for k, fn in link.items()}
                out = dict(format=fmt, direction="host codes to device floats", samples=n, codes_bytes=2 * n, floats_bytes=8 * n)
                out.update({k + "_ms": round(v, 4) for k, v in ms.items()})
                out.update(codes_link_GBps=round(2 * n / ms["unpack_to_device"] / 1e6, 2), floats_link_GBps=round(8 * n / ms["floats_h2d"] / 1e6, 2),
                           codes_of_floats=round(ms["floats_h2d"] / ms["unpack_to_device"], 2))
                print(json.dumps(out), flush=True)
                host_codes.free()
                host_floats.free()
            conv.close()
            del d_codes, d_floats, d_a, d_b
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
