#!/usr/bin/env python3
"""Times of the batched PL stages against the route they replace (notes/plsync_batch.md), HIP-event times on resident buffers, median
of five regions, measured the way tools/plsync_rate.py measures:
  batch     PlSyncBatch search + gather + PlCoarseBatch estimate for S streams: 6 launches and one 8 S byte copy for any S;
  replaced  S single-stream PlSync / PlCoarse handles called one after the other on ONE HIP stream: search, gather, estimate per stream
            (3 S + 2 S launches; the frame count each estimate needs is taken from a warm-up pass, so no host wait is timed).
S = 1, 8 and 64 streams of 2^20 symbols, once LOCKED (clean short QPSK 1/4 frames with pilots behind a random lead, every stream at
another offset) and once SEARCHING throughout (noise of a quarter of unit power: the metric never reaches the threshold). Every handle
is reset in front of every region, outside the events. Prints one markdown table row per case."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, regions, before):
    import torch
    ms = []
    for _ in range(regions):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=1 << 20, help="symbols per stream")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--regions", type=int, default=5)
    args = ap.parse_args()
    import torch
    import plframe_model as M
    import plsync_model as P
    from dvbs2rx_amd import PlCoarse, PlCoarseBatch, PlSync, PlSyncBatch
    st = torch.cuda.current_stream().cuda_stream
    N, rng = args.symbols, np.random.default_rng(1)
    plsc = P.plsc_of(1, 1, 1)
    flen = M.pls_parse(plsc)["plframe_len"]
    slot = flen + 90
    max_frames = N // flen + 8
    s_max = max(args.streams)
    frame = M.make_plframes(plsc, 0, 1, rng)[0].reshape(-1)
    step = 37  # stream s starts `step * s` symbols further into the lead: its frames lie at another offset
    base = np.concatenate([P.qpsk(rng, 1000 + step * s_max), np.tile(frame, N // flen + 2)]).astype(np.complex64)
    d_base = torch.from_numpy(base.view(np.float32).reshape(-1, 2)).cuda()
    print("| streams | state | records per stream | batch: search + gather + coarse, ms | replaced route, ms | replaced / batch |")
    print("| --- | --- | --- | --- | --- | --- |")
    for S in args.streams:
        for what in ("locked", "searching"):
            if what == "locked":
                d_x = torch.stack([d_base[step * (s_max - s):step * (s_max - s) + N] for s in range(S)]).contiguous()
            else:
                d_x = torch.randn((S, N, 2), device="cuda", dtype=torch.float32) * 0.35
            pb = PlSyncBatch(plsc=-1, max_streams=S, max_symbols=N, max_frames=max_frames)
            cb = PlCoarseBatch(1, plsc, max_streams=S, max_slots=S * max_frames)
            d_fb = torch.zeros(S * max_frames * 16, dtype=torch.uint8, device="cuda")
            d_slots = torch.empty(S * max_frames * slot * 2, dtype=torch.float32, device="cuda")
            d_off = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
            d_fo, d_cc = torch.zeros(S * max_frames, device="cuda"), torch.zeros(S * max_frames, dtype=torch.int32, device="cuda")
            first, n_syms = [0] * S, [N] * S

            def batch():
                pb.work_device(d_x.data_ptr(), N, first, n_syms, d_fb.data_ptr(), st)
                pb.gather_device(d_x.data_ptr(), N, d_fb.data_ptr(), S, plsc, d_slots.data_ptr(), S * max_frames, d_off.data_ptr(), 0, st)
                cb.work_device(d_slots.data_ptr(), slot, d_off.data_ptr(), S, 0, d_fo.data_ptr(), d_cc.data_ptr(), 0, st)

            def reset_batch():
                pb.reset()
                cb.reset()

            singles = [(PlSync(plsc=-1, max_symbols=N, max_frames=max_frames), PlCoarse(1, plsc, max_frames=max_frames)) for _ in range(S)]
            d_fs = torch.zeros(S * max_frames * 16, dtype=torch.uint8, device="cuda")
            d_fr = torch.empty(S * (max_frames * flen + 90) * 2, dtype=torch.float32, device="cuda")
            d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
            d_fo1, d_cc1 = torch.zeros(S * max_frames, device="cuda"), torch.zeros(S * max_frames, dtype=torch.int32, device="cuda")
            counts = [0] * S

            def replaced():
                for s, (ps, pc) in enumerate(singles):
                    x, f, fr = d_x.data_ptr() + 8 * N * s, d_fs.data_ptr() + 16 * max_frames * s, d_fr.data_ptr() + 8 * (max_frames * flen + 90) * s
                    ps.work_device(x, N, f, st)
                    ps.gather_device(x, f, max_frames, plsc, fr, d_cnt.data_ptr() + 4 * s, st)
                    pc.work_device(fr, flen, counts[s], 0, d_fo1.data_ptr() + 4 * max_frames * s, d_cc1.data_ptr() + 4 * max_frames * s, 0, st)

            def reset_singles():
                for ps, pc in singles:
                    ps.reset()
                    pc.reset()

            # warm-up: loads the code objects, gives the replaced route its frame counts and checks that the two routes agree
            reset_batch()
            batch()
            nf, _, state = pb.finish()
            reset_singles()
            replaced()
            torch.cuda.synchronize()
            counts = d_cnt.cpu().tolist()
            off = d_off.cpu().tolist()
            assert [b - a for a, b in zip(off[:-1], off[1:])] == counts, (off, counts)
            assert d_fb.cpu().numpy().tobytes() == d_fs.cpu().numpy().tobytes(), "the records of the two routes differ"
            assert set(state.tolist()) == ({2} if what == "locked" else {0}), state
            t_b = timed(batch, args.regions, reset_batch)
            t_r = timed(replaced, args.regions, reset_singles)
            print(f"| {S} | {what} | {int(nf[0])} | {t_b:.3f} | {t_r:.3f} | {t_r / t_b:.2f} |", flush=True)
            for o in [pb, cb] + [h for pair in singles for h in pair]:
                o.close()
            del d_x, d_slots, d_fr


if __name__ == "__main__":
    main()
