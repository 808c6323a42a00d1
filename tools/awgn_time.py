#!/usr/bin/env python3
"""Timings for notes/awgn.md, to be run on an MI355X: the AWGN channel stage (dvbs2_awgn_add_device) on 1 stream of 2^26 samples with
the handle's sigma and on 4096 streams of 32400 samples with a sigma per stream, in place, out of place and the noise alone, each the
median of HIP-event regions after one warm-up, next to, on the same buffers in the same run,
  copy     a plain device-to-device copy of the same bytes (8 in and 8 out per sample: what the out-of-place stage moves),
  torch    the route the stage replaces (tools/fer_device.py --noise torch): torch.randn of the shape, then add_ with one alpha -- a
           noise tensor as large as the signal written and read back, three passes over the bytes and one sigma per call.
Prints one JSON line per shape with the three times and their ratios. Asserts nothing."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

SHAPES = [(1, 1 << 26, False), (4096, 32400, True)]  # (streams, samples per stream, a sigma per stream)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples per stream (a quick look)")
    ap.add_argument("--regions", type=int, default=7)
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import Awgn, capi
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    for streams, per_stream, per_row in SHAPES:
        n = max(1, int(per_stream * a.scale))
        awgn = Awgn(1, 0.5, max_streams=streams, max_samples=n)
        d_in = torch.randn((streams, n, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty_like(d_in)
        d_sig = torch.linspace(0.1, 1.0, streams, dtype=torch.float32, device="cuda") if per_row else None
        sig = d_sig.data_ptr() if per_row else 0
        calls = dict(
            stage_in_place=lambda: awgn.work_device(d_out.data_ptr(), n, n, streams, d_out.data_ptr(), n, 0, 0, sig, st),
            stage_out_of_place=lambda: awgn.work_device(d_in.data_ptr(), n, n, streams, d_out.data_ptr(), n, 0, 0, sig, st),
            stage_noise_only=lambda: awgn.work_device(0, n, n, streams, d_out.data_ptr(), n, 0, 0, sig, st),
            copy=lambda: d_out.copy_(d_in),
            torch_randn_add=lambda: d_out.add_(torch.randn((streams, n, 2), dtype=torch.float32, device="cuda", generator=gen), alpha=0.5))
        d_out.copy_(d_in)
        ms = {k: median_ms(f, a.regions) for k, f in calls.items()}
        awgn.close()
        samples = streams * n
        out = dict(streams=streams, samples_per_stream=n, sigma_per_stream=per_row, tile=capi.AWGN_TILE, bytes_in_plus_out=16 * samples)
        out.update({k + "_ms": v for k, v in ms.items()})
        out.update(stage_Gsamples_per_s=samples / ms["stage_in_place"] / 1e6, stage_GBps=16 * samples / ms["stage_in_place"] / 1e6,
                   noise_only_GBps_written=8 * samples / ms["stage_noise_only"] / 1e6, copy_GBps=16 * samples / ms["copy"] / 1e6,
                   stage_of_copy=ms["copy"] / ms["stage_in_place"], stage_of_torch=ms["torch_randn_add"] / ms["stage_in_place"],
                   torch_of_copy=ms["copy"] / ms["torch_randn_add"])
        print(json.dumps(out), flush=True)
        del d_in, d_out, d_sig
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
