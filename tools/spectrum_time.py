#!/usr/bin/env python3
"""Timings for notes/spectrum.md, to be run on an MI355X: the spectrum stage (dvbs2_spectrum_process_device) at nfft 1024 and 8192 with
the Hann window and hop nfft / 2, avg = 0, on
  1 stream of 2^24 samples;
  1024 streams of 2^14 samples,
each the median of five HIP-event regions after one warm-up, next to, in the same run,
  copy     a plain 16-byte-per-lane copy of the same input bytes (dvbs2_rotator_measure's copy kernel);
  torch    the route the stage replaces: unfold into overlapping segments, the window, torch.fft.fft, abs() ** 2 and mean over the
           segments (the same scale applied once at the end).
Prints one JSON line per case with input samples per second, the ratios to the copy and to the torch route, and the float operations
per second the graph implies (10 per butterfly of a stage with a product, 2 per sample for the window, 3 for the power and 1 for the
sum) against the non-fused float32 VALU peak. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CASES = [(1024, 1, 1 << 24), (1024, 1024, 1 << 14), (8192, 1, 1 << 24), (8192, 1024, 1 << 14)]  # (nfft, streams, samples per stream)
VALU_PEAK = 157.3e12 / 2  # float32 operations per second without fused multiply-add (MI355X: 157.3 TFLOPS counts an FMA as two)


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
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples per stream (a quick look)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch route")
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import Spectrum, capi, spectrum_window
    st = torch.cuda.current_stream().cuda_stream
    for nfft, streams, per_stream in CASES:
        n = max(nfft, int(per_stream * a.scale))
        hop = nfft // 2
        sp = Spectrum(nfft, hop, 0, "hann", True, max_streams=streams, max_samples=n)
        n_seg, n_rows, _ = sp.geometry(n)
        d_in = torch.randn((streams, n, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty((streams, nfft), dtype=torch.float32, device="cuda")
        t = median_ms(lambda: sp.work_device(d_in.data_ptr(), n, n, streams, d_out.data_ptr(), nfft, st))
        power = sp.window_power
        sp.close()
        log2 = nfft.bit_length() - 1
        flops = float(streams) * n_seg * nfft * (2 + 5.0 * (log2 - 1) + 2 + 3 + 1)  # window, butterflies (stage 1: 4 additions), power, sum
        moved = 8 * streams * n
        row = dict(nfft=nfft, streams=streams, samples_per_stream=n, hop=hop, segments_per_stream=n_seg, bytes_in=moved, spectrum_ms=t,
                   spectrum_input_samples_per_s=streams * n / t * 1e3, spectrum_GBps=moved / t / 1e6, spectrum_flops_per_s=flops / t * 1e3,
                   spectrum_share_of_valu_peak=flops / t * 1e3 / VALU_PEAK, lib=os.path.basename(capi.LIB_PATH))
        if not a.no_torch:
            x = torch.view_as_complex(d_in)
            w = torch.from_numpy(spectrum_window("hann", nfft)).cuda()
            scale = 1.0 / power

            def torch_route():
                seg = x.unfold(1, nfft, hop)  # (streams, n_seg, nfft), a view
                p = torch.fft.fft(seg * w, dim=-1).abs() ** 2
                d_out.copy_(torch.fft.fftshift(p.mean(dim=1), dim=-1) * scale)
            try:
                tt = median_ms(torch_route)
                row.update(torch_ms=tt, spectrum_of_torch=tt / t)
            except Exception as e:  # (a shape the library cannot run is a finding, not a crash of the tool)
                row.update(torch_error=str(e)[:200])
            del x, w
        r, c = C.c_double(), C.c_double()
        capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 8, 5, C.byref(r), C.byref(c)))  # reads the input's bytes and writes as many
        row.update(copy_ms=c.value, copy_GBps=2 * moved / c.value / 1e6, spectrum_of_copy=c.value / t)
        del d_in, d_out
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
