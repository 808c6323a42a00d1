#!/usr/bin/env python3
"""Frame and bit error rate of a MODCOD with every frame distinct and everything resident in HBM: random BBFRAME bytes -> FecEncoder
(scrambler on) -> AWGN added on the device with torch (fixed seed) -> FecChain.work_device (descrambler on) -> compared on the
device. Only the error counts come back to the host. A tool, not a test: it asserts no error rate.

--noise device takes the noise from the library's own channel stage (Awgn, dvbs2_awgn_add_device) in place on the symbols: one row per
frame, the stream id the running frame number, so a frame's noise is a function of (--seed, frame number) alone and the counts do not
depend on --batch (the frame's bytes are then a function of the same two as well). Every failed frame is named on stderr with the
(seed, stream id) that regenerates its noise. With --pl the PLFRAME stream is one row, stream id 0, with a running first_index.
--noise torch (the default) is the path above, unchanged.

--pl pilots | nopilots puts the physical layer in between: FecEncoder -> PlFramer (the batch as a CCM sequence plus a closing header,
PL scrambling code --gold) -> AWGN on the whole PLFRAME stream, headers and pilots included -> PlFrontEnd.work_device (trailing header,
frames coarse-corrected: PLSC decoding, pilot / header phase estimates, de-rotation, descrambling) -> FecChain. The JSON line then also
counts the frames whose decoded PLSC was wrong. --pl off (the default) is the path above, unchanged.

--iq u8 | s8 | s16 puts the IQ sample converter (IqConverter, dvbs2_iqconv_*) behind the channel: its output is packed to these codes,
with full scale --iq-backoff dB above the unit symbol amplitude, and unpacked again on the device before the receiver, as a capture in
that format would leave it. The JSON line then also gives the clipped components and their share from the stage's statistics, so the
loss of an 8-bit capture at a given back-off can be read off. Without --iq the tool behaves as before.

  python tools/fer_device.py --rate C1_2 --constellation qpsk --esn0 1.2 --frames 1000000 --batch 4096
  python tools/fer_device.py --rate C1_2 --constellation qpsk --esn0 1.2 --frames 100000 --batch 4096 --pl pilots --gold 5
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

# MODCOD numbers of EN 302 307-1 table 12, in order from 1
MODCODS = ([("qpsk", r) for r in ("C1_4", "C1_3", "C2_5", "C1_2", "C3_5", "C2_3", "C3_4", "C4_5", "C5_6", "C8_9", "C9_10")] +
           [("8psk", r) for r in ("C3_5", "C2_3", "C3_4", "C5_6", "C8_9", "C9_10")] +
           [("16apsk", r) for r in ("C2_3", "C3_4", "C4_5", "C5_6", "C8_9", "C9_10")] +
           [("32apsk", r) for r in ("C3_4", "C4_5", "C5_6", "C8_9", "C9_10")])


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
    ap.add_argument("--pl", choices=("off", "pilots", "nopilots"), default="off", help="frame into PLFRAMEs and receive through PlFrontEnd")
    ap.add_argument("--gold", type=int, default=0, help="PL scrambling code (with --pl)")
    ap.add_argument("--noise", choices=("torch", "device"), default="torch", help="device: the library's AWGN stage, reproducible per frame")
    ap.add_argument("--iq", choices=("u8", "s8", "s16"), default=None, help="pack the channel output to these codes and unpack it again")
    ap.add_argument("--iq-backoff", type=float, default=12.0, metavar="DB", help="full scale above the unit symbol amplitude, in dB (with --iq)")
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import Awgn, FecChain, FecEncoder, IqConverter, PlFramer, PlFrontEnd, capi
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
    plsc_err = torch.zeros((), dtype=torch.int64, device="cuda")
    if a.pl != "off":
        if (a.constellation, a.rate) not in MODCODS:
            sys.exit(f"--pl: DVB-S2 has no MODCOD for {a.constellation} {a.rate}")
        plsc = ((MODCODS.index((a.constellation, a.rate)) + 1) << 2) | ((a.framesize == "short") << 1) | (a.pl == "pilots")
        framer = PlFramer(a.gold, max_frames=batch)
        front = PlFrontEnd(a.gold, plsc, max_frames=batch)
        assert front.xfecframe_len == enc.n_syms
        d_xfec = torch.empty((batch, enc.n_syms, 2), dtype=torch.float32, device="cuda")
        d_pl = torch.empty((batch * front.plframe_len + 90, 2), dtype=torch.float32, device="cuda")
        d_cc = torch.ones((batch,), dtype=torch.int32, device="cuda")
        d_cf = torch.zeros((batch,), dtype=torch.float32, device="cuda")  # read by the pilotless front end only
        d_plsc = torch.empty((batch,), dtype=torch.uint8, device="cuda")
        framed = 0
    if a.noise == "device":
        awgn = Awgn(a.seed, sigma, max_streams=batch, max_samples=enc.n_syms if a.pl == "off" else batch * front.plframe_len + 90)
        byte_of = torch.arange(enc.in_bytes, dtype=torch.int64, device="cuda").view(1, -1)

        def frame_bytes(first, count):  # a 64-bit mix of (seed, frame number, byte number): the same bytes however the frames are batched
            x = torch.arange(first, first + count, dtype=torch.int64, device="cuda").view(-1, 1) * enc.in_bytes + byte_of + a.seed * 0x632BE5AB
            for mul, shift in ((-7046029254386353131, 31), (-4658895280553007687, 29), (-7723592293110705685, 32)):
                x = (x * mul) ^ ((x * mul) >> shift)
            return ((x >> 24) & 255).to(torch.uint8)
    if a.iq:
        iq_rows, iq_max = (batch, enc.n_syms) if a.pl == "off" else (1, batch * front.plframe_len + 90)
        iq_gain = 10.0 ** (-a.iq_backoff / 20.0)
        to_codes = IqConverter(a.iq, iq_gain, max_streams=iq_rows, max_samples=iq_max)
        from_codes = IqConverter(a.iq, 1.0 / iq_gain, max_streams=iq_rows, max_samples=iq_max)
        d_codes = torch.empty(iq_rows * iq_max * to_codes.bytes, dtype=torch.uint8, device="cuda")
        d_iq_stats = torch.zeros((iq_rows, 3), dtype=torch.int64, device="cuda")  # {samples, clipped, energy} per row, added to by every batch

        def through_codes(d_buf, n, rows):  # what an ADC or a recording of this format leaves of the channel output, in place
            to_codes.pack_device(d_buf.data_ptr(), n, n, rows, d_codes.data_ptr(), n, d_stats=d_iq_stats.data_ptr(), stream=st)
            from_codes.unpack_device(d_codes.data_ptr(), n, n, rows, d_buf.data_ptr(), n, stream=st)
    done, t0 = 0, time.time()
    while done < a.frames:
        nf = min(batch, a.frames - done)
        if a.noise == "device":
            d_in = frame_bytes(done, nf)
        else:
            d_in = torch.randint(0, 256, (nf, enc.in_bytes), dtype=torch.uint8, device="cuda", generator=gen)
        if a.pl == "off":
            enc.work_device(d_in.data_ptr(), nf, d_syms=d_syms.data_ptr(), stream=st)
            if a.noise == "device":
                awgn.work_device(d_syms.data_ptr(), enc.n_syms, enc.n_syms, nf, d_syms.data_ptr(), enc.n_syms, first_stream=done, first_index=0, stream=st)
            else:
                d_syms[:nf].add_(torch.randn((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda", generator=gen), alpha=sigma)
            if a.iq:
                through_codes(d_syms, enc.n_syms, nf)
        else:
            if framed != nf:  # the last batch may be shorter
                framer.set_sequence([plsc] * nf)
                framed = nf
            n_pl = nf * front.plframe_len + 90
            enc.work_device(d_in.data_ptr(), nf, d_syms=d_xfec.data_ptr(), stream=st)
            framer.work_device(d_xfec.data_ptr(), nf, plsc, d_pl.data_ptr(), st)
            if a.noise == "device":
                awgn.work_device(d_pl.data_ptr(), n_pl, n_pl, 1, d_pl.data_ptr(), n_pl, first_stream=0, stream=st)  # the running position
            else:
                d_pl[:n_pl].add_(torch.randn((n_pl, 2), dtype=torch.float32, device="cuda", generator=gen), alpha=sigma)
            if a.iq:
                through_codes(d_pl, n_pl, 1)
            front.work_device(d_pl.data_ptr(), nf, 1, d_cc.data_ptr(), d_cf.data_ptr(), d_syms.data_ptr(), st, plsc_decoded=d_plsc.data_ptr())
            plsc_err += (d_plsc[:nf] != plsc).sum()
        chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), 0, d_corr.data_ptr(), st)
        diff = popcount[(d_msg[:nf] ^ d_in).long()].sum(dim=1)
        frame_err += (diff != 0).sum()
        bit_err += diff.sum()
        bch_fail += (d_corr[:nf] < 0).sum()
        if a.noise == "device" and a.pl == "off":
            for f in torch.nonzero(diff).view(-1).tolist():
                print(f"failed frame: seed {a.seed} stream_id {done + f} ({int(diff[f])} bit errors)", file=sys.stderr)
        done += nf
    torch.cuda.synchronize()
    dt = time.time() - t0
    fe, be = int(frame_err.item()), int(bit_err.item())
    out = dict(framesize=a.framesize, rate=a.rate, constellation=a.constellation, esn0_db=a.esn0, frames=done, batch=batch,
               seed=a.seed, frame_errors=fe, bit_errors=be, bch_failures=int(bch_fail.item()), fer=fe / done,
               ber=be / (done * enc.in_bits), seconds=dt, frames_per_s=done / dt)
    if a.noise == "device":
        out.update(noise="device")
        awgn.close()
    if a.iq:
        samples, clipped, energy = (int(v) for v in d_iq_stats.sum(dim=0).tolist())  # (the energy of a run stays far below 2^63)
        unit = 256 if a.iq == "u8" else 128 if a.iq == "s8" else 32768
        out.update(iq=a.iq, iq_backoff_db=a.iq_backoff, iq_clipped=clipped, iq_clipped_share=clipped / (2 * samples),
                   iq_rms_of_full_scale=(energy / samples) ** 0.5 / unit)
        print(f"iq {a.iq}: {clipped} of {2 * samples} components clipped ({100.0 * clipped / (2 * samples):.4f} %), "
              f"rms {(energy / samples) ** 0.5 / unit:.4f} of full scale", file=sys.stderr)
        to_codes.close()
        from_codes.close()
    if a.pl != "off":
        out.update(pl=a.pl, gold=a.gold, plsc=plsc, plsc_errors=int(plsc_err.item()))
        framer.close()
        front.close()
    print(json.dumps(out))
    enc.close()
    chain.close()


if __name__ == "__main__":
    main()
