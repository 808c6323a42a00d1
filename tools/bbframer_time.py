#!/usr/bin/env python3
"""Timings for notes/bbframer.md, to be run on an MI355X: frames/s and bytes/s of the BB framer (TS packets -> BBFRAMEs, one launch
per call, largest DATAFIELD) for QPSK 1/4 short (kbch 3072) and 9/10 normal (kbch 58192), 4096 frames in one call and the same frames in
64 calls of 64, each the median of five event regions after one warm-up (a region holds several repetitions: one call of the short row
is tens of microseconds), next to, in the same run,
  copy     a plain 16-byte-per-lane copy that moves the same number of bytes as the framer reads plus writes (dvbs2_rotator_measure's
           copy kernel);
  encoder  the full encode of the same row (BBFRAME bytes -> QPSK symbols, scrambler on), timed as tools/enc_time.py times it, and
           also in calls of 64;
  serial   the framer with the simple CRC (one lane per CRC slot, 187 dependent table steps; DVBS2_BBFRAMER_CRC=serial when the
           handle is created) instead of sixteen lanes per slot.
Prints one JSON line per row; framer_of_encoder is the framer's frames/s over the encoder's (the condition: >= 1 on both rows), for
one call each, for calls of 64 each, and for the framer in calls of 64 against the encoder in one call."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))

CONFIGS = [("qpsk_1_4_short", 0, "C1_4", 4096), ("qpsk_9_10_normal", 1, "C9_10", 4096)]
SMALL = 64


def median_ms(fn, regions=5, reps=1):
    """median over the regions of the time of ONE fn()"""
    import torch
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / reps)
    return sorted(t)[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the frame counts (a quick look)")
    ap.add_argument("--reps", type=int, default=20, help="framer calls per timed region")
    a = ap.parse_args()
    import torch
    from dvbs2rx_amd import BbFramer, FecEncoder, capi
    st = torch.cuda.current_stream().cuda_stream
    for name, fs, rate, frames in CONFIGS:
        nf = max(SMALL, int(frames * a.scale) // SMALL * SMALL)
        out = dict(config=name, frames=nf)
        d_bb = None
        for variant in ("wave", "serial"):
            os.environ.pop("DVBS2_BBFRAMER_CRC", None)
            if variant == "serial":
                os.environ["DVBS2_BBFRAMER_CRC"] = "serial"
            fr = BbFramer(capi.STANDARD_DVBS2, fs, rate, max_frames=nf)
            os.environ.pop("DVBS2_BBFRAMER_CRC", None)
            # the stream goes on from call to call (a call reads need() packets, one more or less from call to call): the buffers hold the most
            d_ts = torch.randint(0, 256, (fr.max_packets_per_call + 1, 188), dtype=torch.uint8, device="cuda")
            d_ts[:, 0] = 0x47
            d_bb = torch.empty((nf, fr.kbch_bytes), dtype=torch.uint8, device="cuda")
            per_small = -(-SMALL * fr.max_dfl_bytes // 188)

            def one_call():
                fr.work_device(d_ts.data_ptr(), nf, d_bb.data_ptr(), 0, st)

            def small_calls():
                for i in range(nf // SMALL):
                    fr.work_device(d_ts.data_ptr() + i * (per_small - 1) * 188, SMALL, d_bb[i * SMALL].data_ptr(), 0, st)

            t1 = median_ms(one_call, reps=a.reps)
            t64 = median_ms(small_calls, reps=max(1, a.reps // 4))
            moved = nf * (fr.max_dfl_bytes + fr.kbch_bytes)
            c = fr.counters(st)
            assert c["sync_errors"] == 0 and c["bbframes"] > 0
            key = "framer" if variant == "wave" else "serial"
            out.update({key + "_ms": t1, key + "_fps": nf / t1 * 1e3, key + "_GBps": moved / t1 / 1e6,
                        key + "_calls_of_64_ms": t64, key + "_calls_of_64_fps": nf / t64 * 1e3})
            out.update(kbch_bytes=fr.kbch_bytes, bytes_moved=moved)
            fr.close()
            del d_ts
        r, c = C.c_double(), C.c_double()
        capi.check(capi.lib.dvbs2_rotator_measure(0, out["bytes_moved"] // 16, 5, C.byref(r), C.byref(c)))
        out.update(copy_ms=c.value, copy_fps=nf / c.value * 1e3, copy_GBps=out["bytes_moved"] / c.value / 1e6,
                   framer_of_copy=c.value / out["framer_ms"])
        enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, capi.MOD_QPSK, max_frames=nf)
        enc.set_scramble(True)
        d_syms = torch.empty((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda")
        t_enc = median_ms(lambda: enc.work_device(d_bb.data_ptr(), nf, d_syms=d_syms.data_ptr(), stream=st))

        def small_encodes():
            for i in range(nf // SMALL):
                enc.work_device(d_bb[i * SMALL].data_ptr(), SMALL, d_syms=d_syms[i * SMALL].data_ptr(), stream=st)

        t_enc64 = median_ms(small_encodes)
        enc.close()
        out.update(encode_ms=t_enc, encode_fps=nf / t_enc * 1e3, encode_calls_of_64_ms=t_enc64, encode_calls_of_64_fps=nf / t_enc64 * 1e3,
                   framer_of_encoder=t_enc / out["framer_ms"], framer_of_encoder_calls_of_64=t_enc64 / out["framer_calls_of_64_ms"],
                   framer_calls_of_64_of_encoder_one_call=t_enc / out["framer_calls_of_64_ms"],
                   serial_of_framer=out["framer_ms"] / out["serial_ms"],
                   serial_of_framer_calls_of_64=out["framer_calls_of_64_ms"] / out["serial_calls_of_64_ms"])
        print(json.dumps(out), flush=True)
        del d_bb, d_syms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
