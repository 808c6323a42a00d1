#!/usr/bin/env python3
"""Timings for notes/encoder.md, to be run on an MI355X: frames/s of the full encode (BBFRAME bytes -> symbols, scrambler on) for
QPSK 1/2 normal x 4096, 8PSK 3/4 normal x 4096 and QPSK 1/4 short x 16384, each the median of five event regions after one warm-up,
next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the same number of bytes as the encoder reads plus writes (dvbs2_rotator_measure's
           copy kernel: 8 bytes in and 8 bytes out per element);
  decode   dvbs2_chain_decode_device of the encoder's own noiseless output;
  stages   the encode asked for the BCH codeword only, and for the LDPC codeword only (BCH + LDPC): the stage times by difference, and
           the fraction of the copy's bytes/s that each stage reaches on its own input plus output bytes.
Prints one JSON line per configuration. The kernel split comes from `rocprofv3 --kernel-trace --stats -- python tools/enc_time.py`."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CONFIGS = [("qpsk_1_2_normal", 1, "C1_2", 0, 4096), ("8psk_3_4_normal", 1, "C3_4", 4, 4096), ("qpsk_1_4_short", 0, "C1_4", 0, 16384)]


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
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the frame counts (a quick look)")
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import FecChain, FecEncoder, capi
    st = torch.cuda.current_stream().cuda_stream
    for name, fs, rate, mod, frames in CONFIGS:
        nf = max(1, int(frames * a.scale))
        enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, mod, max_frames=nf)
        enc.set_scramble(True)
        kb, bb, lb, sb = enc.in_bytes, enc.bch_n // 8, enc.ldpc_n // 8, enc.n_syms * 8
        d_in = torch.randint(0, 256, (nf, kb), dtype=torch.uint8, device="cuda")
        d_bch = torch.empty((nf, bb), dtype=torch.uint8, device="cuda")
        d_ldpc = torch.empty((nf, lb), dtype=torch.uint8, device="cuda")
        d_syms = torch.empty((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda")
        t_all = median_ms(lambda: enc.work_device(d_in.data_ptr(), nf, d_syms=d_syms.data_ptr(), stream=st))
        t_bch = median_ms(lambda: enc.work_device(d_in.data_ptr(), nf, d_bch_cw=d_bch.data_ptr(), stream=st))
        t_bl = median_ms(lambda: enc.work_device(d_in.data_ptr(), nf, d_ldpc_cw=d_ldpc.data_ptr(), stream=st))
        moved = nf * (kb + sb)
        r, c = C.c_double(), C.c_double()
        capi.check(capi.lib.dvbs2_rotator_measure(0, moved // 16, 5, C.byref(r), C.byref(c)))
        copy_gbps = moved / c.value / 1e6
        stages = {"bch": (t_bch, kb + bb), "ldpc": (t_bl - t_bch, bb + lb), "mapper": (t_all - t_bl, lb + sb), "whole": (t_all, kb + sb)}
        out = dict(config=name, frames=nf, encode_ms=t_all, encode_fps=nf / t_all * 1e3, copy_ms=c.value, copy_fps=nf / c.value * 1e3,
                   copy_GBps=copy_gbps, bytes_per_frame=kb + sb)
        for k, (ms, nbytes) in stages.items():
            out[k + "_ms"] = ms
            out[k + "_of_copy"] = (nf * nbytes / ms / 1e6) / copy_gbps if ms > 0 else None
        if not a.no_decode:
            chain = FecChain(capi.STANDARD_DVBS2, fs, rate, mod, group_size=32, max_frames=nf)
            chain.set_descramble(True)
            d_n0 = torch.full((1,), 0.02, dtype=torch.float32, device="cuda")
            d_msg = torch.empty((nf, kb), dtype=torch.uint8, device="cuda")
            d_corr = torch.empty((nf,), dtype=torch.int32, device="cuda")
            t_dec = median_ms(lambda: chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), 0, d_corr.data_ptr(), st))
            out.update(decode_ms=t_dec, decode_fps=nf / t_dec * 1e3, loopback_equal=bool(torch.equal(d_msg, d_in)),
                       bch_corrections=int(d_corr.abs().sum().item()))
            chain.close()
        enc.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
