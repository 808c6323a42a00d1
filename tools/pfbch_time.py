#!/usr/bin/env python3
"""Timings for notes/pfbch.md, to be run on an MI355X: the polyphase channelizer (dvbs2_pfbch_process_device) on 1 stream of 2^24 samples
with M = 8, 16 and 64 channels, D = M / 2, 16 M + 1 taps, all channels selected and a quarter of them, each the median of five HIP-event
regions after one warm-up, next to, in the same run,
  copy     (a) a plain 16-byte-per-lane copy that moves the input bytes once plus the output bytes (dvbs2_rotator_measure's copy kernel);
  ddc      (b) the route the stage replaces: Ddc with the same taps and D and phase_inc = -2 pi c / M on as many channels as are selected;
  torch    (c) unfold over the zero-padded input, a product with the taps and a sum per branch (the matmul of the polyphase form), the
           rotation of the residues, torch.fft.fft and the transpose into rows; skipped with its error where it does not fit in memory.
Prints one JSON line per case with input samples per second and the bytes per second against the copy. Asserts nothing."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CASES = [(M, quarter) for M in (8, 16, 64) for quarter in (False, True)]


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


def lowpass(M, ntaps):
    import numpy as np
    return (np.sinc((np.arange(ntaps) - (ntaps - 1) / 2) / M) * np.hamming(ntaps) / M).astype(np.float32)


def make_torch_route(x, taps, M, D, sel):
    """Route (c) as a function without arguments: x a complex64 tensor of n samples (n a multiple of D, D a divisor of M) from a counter of
    zero, on any device. Returns complex64 [len(sel), n / D]. tests/test_pfbch_model.py holds it against the float64 model."""
    import numpy as np
    import torch
    ntaps, n_out = len(taps), x.numel() // D
    q = -(-ntaps // M)
    L = q * M
    h = np.zeros(L, np.float32)
    h[:ntaps] = taps
    # frame k holds the samples k D - L + 1 .. k D; the tap of its element e is L - 1 - e
    hm = torch.from_numpy(h[::-1].copy()).to(x.device).reshape(q, M).to(torch.complex64)
    xp = torch.cat([torch.zeros(L - 1, dtype=torch.complex64, device=x.device), x])
    idx = torch.tensor(sel, device=x.device)

    def torch_route():
        frames = xp.unfold(0, L, D)[:n_out].reshape(n_out, q, M)
        w = (frames * hm).sum(dim=1)  # element m of frame k has the residue (k D + 1 + m) mod M
        for phase in range(M // D):
            w[phase::M // D] = torch.roll(w[phase::M // D], shifts=(phase * D + 1) % M, dims=1)
        y = torch.fft.fft(w, dim=1)
        return y.t()[idx].contiguous()

    return torch_route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the samples (a quick look)")
    ap.add_argument("--no-torch", action="store_true", help="skip route (c)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvbs2rx_amd import Ddc, PfbChannelizer, capi, pfbch_tile
    st = torch.cuda.current_stream().cuda_stream
    for M, quarter in CASES:
        D, ntaps = M // 2, 16 * M + 1
        n = max(M, int((1 << 24) * a.scale)) // M * M
        taps = lowpass(M, ntaps)
        sel = list(range(0, M, 4)) if quarter else list(range(M))
        n_out = n // D  # from a counter that is a multiple of D
        d_in = torch.randn((n, 2), dtype=torch.float32, device="cuda")
        d_out = torch.empty((len(sel) * n_out, 2), dtype=torch.float32, device="cuda")
        ch = PfbChannelizer(M, D, taps, max_samples=n)
        ch.set_channels(sel)

        def pfb_only():
            ch.work_device(d_in.data_ptr(), n, n, 1, d_out.data_ptr(), n_out, st)  # n is a multiple of D and M: every call does the same work

        t = median_ms(pfb_only)
        ch.close()
        moved = 8 * (n + len(sel) * n_out)
        row = dict(n_chan=M, decim=D, ntaps=ntaps, selected=len(sel), samples=n, tile=pfbch_tile(M, D, ntaps), out_samples_per_channel=n_out,
                   bytes_moved=moved, pfbch_ms=t, pfbch_input_samples_per_s=n / t * 1e3, pfbch_GBps=moved / t / 1e6, lib=os.path.basename(capi.LIB_PATH))
        # (a) the copy of its bytes
        r, c = C.c_double(), C.c_double()
        capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
        row.update(copy_ms=c.value, copy_GBps=moved / c.value / 1e6, pfbch_of_copy=c.value / t)
        # (b) the down-converter on the selected channels
        dd = Ddc(D, taps, max_channels=len(sel), max_samples=n)
        for i, chan in enumerate(sel):
            dd.set_channel(i, -2.0 * np.pi * chan / M)
        td = median_ms(lambda: dd.work_device(d_in.data_ptr(), n, n, 1, len(sel), d_out.data_ptr(), n_out, st))
        dd.close()
        row.update(ddc_ms=td, ddc_over_pfbch=td / t)
        # (c) the torch route
        if not a.no_torch:
            try:
                torch_route = make_torch_route(torch.view_as_complex(d_in), taps, M, D, sel)
                tt = median_ms(torch_route)
                row.update(torch_ms=tt, torch_over_pfbch=tt / t)
                del torch_route
            except Exception as e:  # (a shape that does not fit is a finding, not a crash of the tool)
                row.update(torch_error=str(e)[:200])
        del d_in, d_out
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
