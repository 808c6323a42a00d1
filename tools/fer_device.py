#!/usr/bin/env python3
"""Frame and bit error rate of a MODCOD with every frame distinct and everything resident in HBM: random BBFRAME bytes -> FecEncoder
(scrambler on) -> AWGN added on the device with torch (fixed seed) -> FecChain.work_device (descrambler on) -> compared on the
device. Only the error counts come back to the host. A tool, not a test: it asserts no error rate.

  python tools/fer_device.py --rate C1_2 --constellation qpsk --esn0 1.2 --frames 1000000 --batch 4096
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--framesize", choices=("short", "normal"), default="normal")
    ap.add_argument("--rate", default="C1_2")
    ap.add_argument("--constellation", choices=("qpsk", "8psk", "16apsk", "32apsk"), default="qpsk")
    ap.add_argument("--esn0", type=float, required=True, help="Es/N0 in dB (Es = 1)")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--trials", type=int, default=0, help="LDPC iteration cap (0: the reference's 25)")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import FecChain, FecEncoder, capi
    fs = capi.FECFRAME_NORMAL if a.framesize == "normal" else capi.FECFRAME_SHORT
    mod = {"qpsk": capi.MOD_QPSK, "8psk": capi.MOD_8PSK, "16apsk": capi.MOD_16APSK, "32apsk": capi.MOD_32APSK}[a.constellation]
    batch = min(a.batch, a.frames)
    enc = FecEncoder(capi.STANDARD_DVBS2, fs, a.rate, mod, max_frames=batch)
    chain = FecChain(capi.STANDARD_DVBS2, fs, a.rate, mod, group_size=32, max_frames=batch, max_trials=a.trials)
    enc.set_scramble(True)
    chain.set_descramble(True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(a.seed)
    n0 = 10.0 ** (-a.esn0 / 10.0)
    sigma = (n0 / 2.0) ** 0.5
    st = torch.cuda.current_stream().cuda_stream
    d_syms = torch.empty((batch, enc.n_syms, 2), dtype=torch.float32, device="cuda")
    d_n0 = torch.full((1,), n0, dtype=torch.float32, device="cuda")
    d_msg = torch.empty((batch, enc.in_bytes), dtype=torch.uint8, device="cuda")
    d_corr = torch.empty((batch,), dtype=torch.int32, device="cuda")
    popcount = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device="cuda")
    frame_err = torch.zeros((), dtype=torch.int64, device="cuda")
    bit_err = torch.zeros((), dtype=torch.int64, device="cuda")
    bch_fail = torch.zeros((), dtype=torch.int64, device="cuda")
    done, t0 = 0, time.time()
    while done < a.frames:
        nf = min(batch, a.frames - done)
        d_in = torch.randint(0, 256, (nf, enc.in_bytes), dtype=torch.uint8, device="cuda", generator=gen)
        enc.work_device(d_in.data_ptr(), nf, d_syms=d_syms.data_ptr(), stream=st)
        d_syms[:nf].add_(torch.randn((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda", generator=gen), alpha=sigma)
        chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), 0, d_corr.data_ptr(), st)
        diff = popcount[(d_msg[:nf] ^ d_in).long()].sum(dim=1)
        frame_err += (diff != 0).sum()
        bit_err += diff.sum()
        bch_fail += (d_corr[:nf] < 0).sum()
        done += nf
    torch.cuda.synchronize()
    dt = time.time() - t0
    fe, be = int(frame_err.item()), int(bit_err.item())
    print(json.dumps(dict(framesize=a.framesize, rate=a.rate, constellation=a.constellation, esn0_db=a.esn0, frames=done, batch=batch,
                          seed=a.seed, frame_errors=fe, bit_errors=be, bch_failures=int(bch_fail.item()), fer=fe / done,
                          ber=be / (done * enc.in_bits), seconds=dt, frames_per_s=done / dt)))
    enc.close()
    chain.close()


if __name__ == "__main__":
    main()
