#!/usr/bin/env python3
"""Times of the de-header rows against the route they replace and against a copy of their bytes (notes/bbdeheader_rows.md): HIP-event
times on resident buffers, medians over --regions regions, the records reset OUTSIDE the events in front of every region (so every
region does the same work: each stream starts not synchronised and walks its frames in order, both routes alike).
  rows      bbdeheader_rows_device: S streams in FIVE launches from records in device memory, d_offsets read on the device;
  replaced  S single dvbs2_bbdeheader_t handles called one after the other on one stream (4 S launches), WITHOUT the S finish() waits that
            route needs to learn its byte counts. With --parent-lib PATH (default: the environment's DVBS2_LIB, which this tool takes
            for itself) the handles come from THAT library -- libdvbs2_fec_hip.so built from the parent commit, loaded next to the
            product library in the same process -- so that the yardstick is not the code under test;
  copy      a device-to-device copy of (bytes read + bytes written) / 2 bytes: it moves what the rows move;
  empty     one launch of a kernel that does nothing.
Healthy streams: one BbFramer stream of random TS packets over all frames, cut into S streams of equal length (every stream but the first
starts inside a packet and synchronises on its first SYNCD). 4096 frames of kbch 58192 and 65536 frames of kbch 3072 in all, S in 1, 8, 64,
1024. Both routes must give the same bytes. Prints markdown table rows and, per row, how it stands against the expectation
(S = 1: rows <= replaced + the spread of the replaced route's regions + one empty launch; S > 1: rows < replaced). Asserts no time."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_LIB = os.environ.pop("DVBS2_LIB", None)  # the product library is the one under test here; DVBS2_LIB names the yardstick
sys.path.insert(0, os.path.join(ROOT, "gr-dvbs2rx_amd", "python"))


CALL_FRAMES = 32768  # the single handles (de-header and framer) take at most 65535 frames per call: a longer stream goes in calls of this many


def calls_of(n):
    """(first frame, count) of the calls a single handle needs for n frames"""
    return [(f0, min(CALL_FRAMES, n - f0)) for f0 in range(0, n, CALL_FRAMES)]


def timed(fn, reset, regions):
    import torch
    ms = []
    for r in range(-1, regions):  # region -1 warms up
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= 0:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.max(ms) - np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["58192:4096", "3072:65536"], help="kbch_bits:frames in all")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 64, 1024])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--parent-lib", default=PARENT_LIB, help="libdvbs2_fec_hip.so of the parent commit: the replaced route")
    args = ap.parse_args()
    import torch
    from dvbs2rx_amd import BBDEHEADER_STATE, BbFramer, bbdeheader_rows_device, bbdeheader_rows_geometry, capi
    assert torch.cuda.is_available(), "a time is a time on the GPU"
    st = torch.cuda.current_stream().cuda_stream
    old = capi.lib
    names = ("dvbs2_bbdeheader_create_raw", "dvbs2_bbdeheader_destroy", "dvbs2_bbdeheader_process_device", "dvbs2_bbdeheader_finish", "dvbs2_bbdeheader_reset")
    if args.parent_lib:
        old = C.CDLL(os.path.abspath(args.parent_lib))
        for name in names:
            getattr(old, name).restype, getattr(old, name).argtypes = capi.SYMBOLS[name]
        assert not hasattr(old, "dvbs2_bbdeheader_rows_device"), "--parent-lib already has the de-header rows: it is not the parent's library"
    print(f"replaced route from {'the parent library ' + args.parent_lib if args.parent_lib else 'the product library itself'}")
    t_empty, sp_empty = timed(lambda: torch.cuda._sleep(0), lambda: None, args.regions)
    print(f"one empty launch: {t_empty * 1e3:.1f} us (spread {sp_empty * 1e3:.1f})")
    for case in args.cases:
        kbch, total = (int(v) for v in case.split(":"))
        kb = kbch // 8
        framer = BbFramer(kbch_bits=kbch, max_frames=min(total, CALL_FRAMES))
        n_ts = total * (kb - 10) // 188 + 2
        d_tspk = torch.randint(0, 256, (n_ts, 188), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(kbch))
        d_tspk[:, 0] = 0x47
        d_bb = torch.zeros(total * kb, dtype=torch.uint8, device="cuda")
        taken = 0
        for f0, c in calls_of(total):  # one stream: the framer carries its position from call to call
            k = framer.need(c)
            assert taken + k <= n_ts
            framer.work_device(d_tspk.data_ptr() + 188 * taken, c, d_bb.data_ptr() + f0 * kb, 0, st)
            taken += k
        torch.cuda.synchronize()
        framer.close()
        print(f"\nkbch {kbch}, {total} frames in all ({total * kb / 2 ** 20:.1f} MiB of BBFRAMEs)")
        print("| S | frames per stream | rows, ms | spread | replaced (S handles, no finish), ms | spread | copy, ms | rows / copy | replaced / rows | expectation |")
        print("| --- | --- | --- | --- | --- | --- | --- | --- | --- | --- |")
        for S in args.streams:
            n = total // S
            g = bbdeheader_rows_geometry(kbch, S, total)
            per_frame = g["max_out_bytes_per_frame"]
            d_state = torch.zeros(S * BBDEHEADER_STATE.itemsize, dtype=torch.uint8, device="cuda")
            d_work = torch.zeros(g["work_bytes"], dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(g["out_bytes"], dtype=torch.uint8, device="cuda")
            d_old = torch.zeros(g["out_bytes"], dtype=torch.uint8, device="cuda")
            d_off = torch.arange(0, (S + 1) * n, n, dtype=torch.int32, device="cuda")
            d_pko = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
            handles = []
            for _ in range(S):
                h = C.c_void_p()
                capi.check(old.dvbs2_bbdeheader_create_raw(C.byref(h), kbch, min(n, CALL_FRAMES), 0))
                handles.append(h)

            def rows():
                bbdeheader_rows_device(d_bb.data_ptr(), kbch, d_off.data_ptr(), S, total, d_state.data_ptr(), d_work.data_ptr(), g["work_bytes"],
                                       d_out.data_ptr(), g["out_bytes"], d_pko.data_ptr(), 0, st)

            def rows_reset():
                d_state.zero_()

            def replaced(counts=None):
                # (a stream of more than one call: without a finish() the host does not know where the first call's packets end, so the
                # next call writes at its frames' offset; counts: a list that receives every call's byte count, through finish())
                for s, h in enumerate(handles):
                    for f0, c in calls_of(n):
                        f = s * n + f0
                        capi.check(old.dvbs2_bbdeheader_process_device(h, d_bb.data_ptr() + f * kb, c, d_old.data_ptr() + f * per_frame, st))
                        if counts is not None:
                            produced = C.c_int64()
                            capi.check(old.dvbs2_bbdeheader_finish(h, C.byref(produced), st))
                            counts.append((s, f * per_frame, produced.value))

            def replaced_reset():
                for h in handles:
                    old.dvbs2_bbdeheader_reset(h, st)

            # both routes from the block as constructed: the same bytes per stream
            rows_reset()
            rows()
            replaced_reset()
            counts = []
            replaced(counts)
            torch.cuda.synchronize()
            pko = d_pko.cpu().numpy()
            got, was = d_out.cpu().numpy(), d_old.cpu().numpy()
            for s in range(S):
                one = np.concatenate([was[at:at + nbytes] for s_, at, nbytes in counts if s_ == s])
                assert one.size == 188 * int(pko[s + 1] - pko[s]), f"stream {s}: the two routes give other counts"
                assert np.array_equal(got[188 * int(pko[s]):188 * int(pko[s + 1])], one), f"stream {s}: the two routes differ"
            moved = total * kb + 188 * int(pko[S])
            d_a, d_b = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda"), torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")
            t_rows, sp_rows = timed(rows, rows_reset, args.regions)
            t_rep, sp_rep = timed(replaced, replaced_reset, args.regions)
            t_copy, _ = timed(lambda: d_b.copy_(d_a), lambda: None, args.regions)
            if S == 1:
                margin = sp_rep + t_empty
                verdict = f"{'met' if t_rows <= t_rep + margin else 'NOT met'}: rows - replaced = {(t_rows - t_rep) * 1e3:+.1f} us, margin {margin * 1e3:.1f} us"
            else:
                verdict = "met" if t_rows < t_rep else "NOT met"
            print(f"| {S} | {n} | {t_rows:.4f} | {sp_rows:.4f} | {t_rep:.4f} | {sp_rep:.4f} | {t_copy:.4f} | {t_rows / t_copy:.2f} | {t_rep / t_rows:.2f} | {verdict} |",
                  flush=True)
            if S == 1 and len(calls_of(n)) > 1:
                # The single handle needed several calls for this stream, and only the first of them starts not synchronised: the later
                # ones take the healthy stretch as prefix sums, where one rows call walks the whole stream in order. The rows in the SAME calls:
                d_offs = [torch.tensor([0, c], dtype=torch.int32, device="cuda") for _, c in calls_of(n)]

                def rows_same_calls():
                    for (f0, c), d_o in zip(calls_of(n), d_offs):
                        bbdeheader_rows_device(d_bb.data_ptr() + f0 * kb, kbch, d_o.data_ptr(), 1, c, d_state.data_ptr(), d_work.data_ptr(), g["work_bytes"],
                                               d_out.data_ptr() + f0 * per_frame, g["out_bytes"] - f0 * per_frame, d_pko.data_ptr(), 0, st)

                t_same, sp_same = timed(rows_same_calls, rows_reset, args.regions)
                margin = sp_rep + len(calls_of(n)) * t_empty
                print(f"| 1, in the single handle's {len(calls_of(n))} calls | {CALL_FRAMES} per call | {t_same:.4f} | {sp_same:.4f} | {t_rep:.4f} | {sp_rep:.4f} | | | "
                      f"{t_rep / t_same:.2f} | {'met' if t_same <= t_rep + margin else 'NOT met'}: rows - replaced = {(t_same - t_rep) * 1e3:+.1f} us, margin "
                      f"{margin * 1e3:.1f} us |", flush=True)
            for h in handles:
                old.dvbs2_bbdeheader_destroy(h)


if __name__ == "__main__":
    main()
