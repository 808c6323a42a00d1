#!/usr/bin/env python3
"""Timings for notes/ddc.md, to be run on an MI355X: the down-converter (dvbs2_ddc_process_device) on
  1 input of 2^24 samples, 1 / 16 / 64 channels, D = 8, 129 taps;
  1 input of 2^24 samples, 16 channels, D = 50, 801 taps;
  64 inputs of 2^18 samples with one channel each, D = 4, 65 taps,
each the median of five HIP-event regions after one warm-up, next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the input bytes once plus the output bytes (dvbs2_rotator_measure's copy kernel);
  torch    the route the stage replaces: Rotator per channel into a temporary, the temporary's real and imaginary rows made contiguous,
           then torch.nn.functional.conv1d with stride D over the two rows. Timed on at most --torch-channels channels and scaled to the
           case's channels (the route is a loop over channels: its time is proportional);
  shaper   dvbs2_pulse_shape_device at sps 2 writing as many output samples over as many streams, with the longest filter it takes when
           the down-converter's is longer (129 terms per output sample at most); compared by terms (taps times output samples) per second.
Prints one JSON line per case with input samples x channels per second and the float operations per second the FIR and the mixer's six
operations imply (4 per tap and output sample, 6 per input sample and channel; sincospif not counted) against the non-fused float32 VALU
peak. The share of time outside the FIR loop is this tool's ddc_ms under a library built with -DDVBS2_DDC_ONE_TAP (tools/build_variant.sh,
selected through DVBS2_LIB) over its ddc_ms under the product library. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CASES = [(1, 1 << 24, 1, 8, 129), (1, 1 << 24, 16, 8, 129), (1, 1 << 24, 64, 8, 129), (1, 1 << 24, 16, 50, 801),
         (64, 1 << 18, 64, 4, 65)]  # (inputs, samples per input, channels, D, ntaps)
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


def lowpass(D, ntaps):
    import numpy as np
    return (np.sinc((np.arange(ntaps) - (ntaps - 1) / 2) / D) * np.hamming(ntaps) / D).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples per input (a quick look)")
    ap.add_argument("--torch-channels", type=int, default=4, help="channels the torch route is timed on (0: skip it)")
    ap.add_argument("--only-ddc", action="store_true", help="skip copy, torch and shaper (the one-tap build)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvbs2rx_amd import Ddc, PulseShaper, Rotator, capi
    st = torch.cuda.current_stream().cuda_stream
    for inputs, per_input, channels, D, ntaps in CASES:
        n = max(D, int(per_input * a.scale))
        taps = lowpass(D, ntaps)
        incs = [2 * np.pi * (c + 0.5 - channels / 2) / max(channels, 2) * 0.9 for c in range(channels)]
        dd = Ddc(D, taps, max_channels=channels, max_inputs=inputs, max_samples=n)
        for c in range(channels):
            dd.set_channel(c, incs[c], c % inputs)
        n_out = -(-n // D)  # from a counter that is a multiple of D; other calls write one less at most
        d_in = torch.randn((inputs * n, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty((channels * n_out, 2), dtype=torch.float32, device="cuda")
        t = median_ms(lambda: dd.work_device(d_in.data_ptr(), n, n, inputs, channels, d_out.data_ptr(), n_out, st))
        dd.close()
        moved = 8 * (inputs * n + channels * n_out)
        flops = 4.0 * ntaps * n_out * channels + 6.0 * n * channels
        row = dict(inputs=inputs, samples_per_input=n, channels=channels, decim=D, ntaps=ntaps, tile=min(capi.DDC_MAX_TILE, (capi.DDC_SPAN - ntaps + 1) // D),
                   out_samples_per_channel=n_out, bytes_moved=moved, ddc_ms=t, ddc_input_samples_x_channels_per_s=n * channels / t * 1e3,
                   ddc_GBps=moved / t / 1e6, ddc_flops_per_s=flops / t * 1e3, ddc_share_of_valu_peak=flops / t * 1e3 / VALU_PEAK,
                   lib=os.path.basename(capi.LIB_PATH))
        if not a.only_ddc:
            # (b) the torch route on the first channels, input c % inputs each
            tc = min(channels, a.torch_channels)
            if tc > 0:
                rots = [Rotator(incs[c]) for c in range(tc)]
                d_tmp = torch.empty((n, 2), dtype=torch.float32, device="cuda")
                w = torch.from_numpy(taps[::-1].copy()).cuda().reshape(1, 1, -1)  # conv1d correlates: the taps flipped
                pad = ntaps - 1

                def torch_route():
                    for c in range(tc):
                        x = d_in[(c % inputs) * n:(c % inputs + 1) * n]
                        rots[c].work_device(x.data_ptr(), n, d_tmp.data_ptr(), st)
                        rows = d_tmp.t().contiguous().unsqueeze(1)  # (2, 1, n): real row, imaginary row
                        y = torch.nn.functional.conv1d(rows, w, stride=D, padding=pad)  # output k ends on sample k D, as the stage's
                        d_out[c * n_out:(c + 1) * n_out] = y.squeeze(1)[:, :n_out].t()
                try:
                    tt = median_ms(torch_route)
                    row.update(torch_channels_timed=tc, torch_ms_timed=tt, torch_ms_scaled=tt * channels / tc, ddc_of_torch=tt * channels / tc / t)
                except Exception as e:  # (a convolution of this shape the library cannot run is a finding, not a crash of the tool)
                    row.update(torch_error=str(e)[:200])
                for r in rots:
                    r.close()
                del d_tmp, w
            del d_in, d_out
            torch.cuda.empty_cache()
            # (c) the shaper at sps 2: as many output samples over `channels` streams
            terms = min(ntaps, 129)
            delay = max(1, min(64, (2 * terms - 1) // 4))
            syms = max(1, n_out // 2)
            ps = PulseShaper(2, 0.2, delay, max_streams=channels, max_symbols=syms)
            p_in = torch.randn((channels * syms, 2), dtype=torch.float32, device="cuda")
            p_out = torch.empty((channels * syms * 2, 2), dtype=torch.float32, device="cuda")
            tp = median_ms(lambda: ps.work_device(p_in.data_ptr(), syms, syms, channels, p_out.data_ptr(), syms * 2, st))
            shaper_terms = channels * syms * ps.ntaps  # every symbol meets every tap once
            ps.close()
            del p_in, p_out
            torch.cuda.empty_cache()
            r, c = C.c_double(), C.c_double()
            capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
            ddc_terms = float(ntaps) * n_out * channels
            row.update(copy_ms=c.value, copy_GBps=moved / c.value / 1e6, ddc_of_copy=c.value / t, shaper_rrc_delay=delay, shaper_ntaps=ps.ntaps,
                       shaper_ms=tp, shaper_terms_per_s=shaper_terms / tp * 1e3, ddc_terms_per_s=ddc_terms / t * 1e3,
                       ddc_of_shaper_by_terms=(ddc_terms / t) / (shaper_terms / tp))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
