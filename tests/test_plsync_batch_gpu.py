"""The batched PL stages (dvbs2_plsync_batch_*, dvbs2_plcoarse_batch_*, dvbs2_plframe_*_strided_device) against the single-stream
handles they stand for: per stream every record, count, `consumed`, state, gathered symbol, coarse estimate and XFECFRAME symbol is the
single-stream handle's, bit for bit. The single-stream handles are tied to their float64 models by their own tests; the clean streams
here are compared with tests/plsync_model.py once more. Five streams in one handle (tests/plsync_batch_case.py): three of
loopback.SEQ6 with different seeds and leads, one of them behind noise at 10 dB, one of noise alone, and one that is presented nothing."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import plframe_model as M
import plsync_batch_case as B
import plsync_model as P
from dvbs2rx_amd import FecChain, PlCoarse, PlCoarseBatch, PlFrontEnd, PlSync, PlSyncBatch, Rotator, SymbolSync, capi

pytestmark = pytest.mark.gpu

PLSC, SLOT, FRAME_LEN = B.PLSC, B.SLOT, B.FRAME_LEN
SEQ_STREAMS = (B.CLEAN_A, B.NOISY, B.CLEAN_B)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def compare_with_model(recs, s, what):
    """as compare_records of tests/test_plsync_gpu.py: index, PLSC and flags exactly, the metric within the model's float32 bound"""
    want, _, _, bound = B.model_records(s)
    assert recs["sof_index"].tolist() == [r[0] for r in want] and recs["plsc"].tolist() == [r[2] for r in want]
    assert recs["flags"].tolist() == [r[3] for r in want]
    at = np.array([r[0] + 89 for r in want])
    err = np.abs(recs["metric"].astype(np.float64) - np.array([r[1] for r in want]))
    print(f"{what}: {len(want)} records as the model's, metric worst error / bound {np.max(err / bound[at]):.3f}")
    assert (err <= bound[at]).all()


# ------------------------------------------------------------------ 1. search
@pytest.mark.parametrize("cut", [False, True], ids=["one-call", "cut-per-stream"])
def test_search_equals_single_stream_handles(cut):
    c = B.streams()
    ps = B.make_batch(5)
    got = B.run_batch(ps, c.d_x, c.stride, c.n, {s: B.sizes_of(s) for s in range(5)} if cut else None)
    ps.close()
    print(f"batch of 5 in {got.n_calls} calls; calls per stream {[len(k) for k in got.calls]}, records per stream {[len(r) for r in got.recs]}")
    for s in range(5):
        want = B.single_reference(s, cut)
        assert len(got.calls[s]) == len(want), s
        for i, (g, w) in enumerate(zip(got.calls[s], want)):
            assert g == w, f"stream {s}, call {i}: n_syms, n_frames, consumed, state {g[0], g[2:]} against {w[0], w[2:]} of the single handle" + \
                ("" if g[1] == w[1] else "; the records differ")
    assert got.calls[B.EMPTY] == [] and len(got.recs[B.NOISE_ONLY]) == 0 and got.state[B.NOISE_ONLY] == capi.PLSYNC_SEARCHING
    for s in (B.CLEAN_A, B.CLEAN_B):
        compare_with_model(got.recs[s], s, f"stream {s}" + (" in cut calls" if cut else ""))
        _, consumed, state, _ = B.model_records(s)
        assert (got.pos[s], got.state[s]) == (consumed, state) and state == capi.PLSYNC_LOCKED
        assert [int(r["plsc"]) for r in got.recs[s]] == L.SEQ6
    assert got.state[B.NOISY] == capi.PLSYNC_LOCKED and len(got.recs[B.NOISY]) >= 8  # 10 dB: every frame found, false crossings allowed
    if cut:
        assert len({tuple(k[0] for k in got.calls[s][:2]) for s in SEQ_STREAMS}) == 3  # the streams were cut at different points


def test_streams_do_not_touch_each_other():
    """with and without the noise stream and the empty one; reset_stream(1) restarts stream 1 alone"""
    import torch
    c = B.streams()
    sizes = {s: B.sizes_of(s) for s in range(5)}
    ps = B.make_batch(5)
    full = B.run_batch(ps, c.d_x, c.stride, c.n, sizes)
    d3 = c.d_x[list(SEQ_STREAMS)].contiguous()
    p3 = B.make_batch(3)
    three = B.run_batch(p3, d3, c.stride, [c.n[s] for s in SEQ_STREAMS], {i: sizes[s] for i, s in enumerate(SEQ_STREAMS)})
    p3.close()
    for i, s in enumerate(SEQ_STREAMS):
        assert three.calls[i] == full.calls[s], f"stream {s} changes with the noise stream and the empty stream beside it"
    # the first call of every stream once more, stream 1 behind a reset of its own: it starts again, the others go on where they are
    n1 = [min(c.n[s], sizes[s][0]) for s in range(5)]
    d_f = B.zeros(5 * ps.max_frames * 16, "uint8")
    ps.reset_stream(B.NOISY)
    ps.work_device(c.d_x.data_ptr(), c.stride, [0] * 5, n1, d_f.data_ptr(), T.stream())
    nf, consumed, state = ps.finish()
    recs = B.records(d_f, 5)
    first = full.calls[B.NOISY][0]
    assert (n1[B.NOISY], recs[B.NOISY, :nf[B.NOISY]].tobytes(), nf[B.NOISY], consumed[B.NOISY], state[B.NOISY]) == first
    for s in (B.CLEAN_A, B.CLEAN_B):  # not reset: absolute indices go on from the end of the first pass
        fresh = np.frombuffer(full.calls[s][0][1], PlSync.FRAME_DTYPE)
        assert nf[s] > 0 and (recs[s, :nf[s]]["sof_index"] >= full.pos[s]).all() and recs[s, 0]["sof_index"] != fresh[0]["sof_index"]
    # reset: every stream as created
    ps.reset()
    again = B.run_batch(ps, c.d_x, c.stride, c.n, sizes)
    assert again.calls == full.calls
    ps.close()
    torch.cuda.synchronize()


def test_batch_of_one_stride_and_odd_first():
    """S = 1 is the single handle; a stride larger than the row and odd first values (8-byte aligned sources) give the same bytes"""
    import torch
    c = B.streams()
    s = B.CLEAN_B
    want = B.single_reference(s, True)
    for shift, stride in ((0, c.stride), (1, 3 * c.stride + 1), (7, c.n[s] + 7)):
        d = torch.zeros((c.n[s] + shift + 1) * 2, dtype=torch.float32, device="cuda")
        d[2 * shift:2 * (shift + c.n[s])] = c.d_x[s, :c.n[s]].reshape(-1)
        ps = B.make_batch(1)
        got = B.run_batch(ps, d, stride, [c.n[s]], {0: B.sizes_of(s)}, first0=[shift])
        ps.close()
        assert got.calls[0] == want, (shift, stride)
    # two rows at an odd stride, the second presented from an odd first: row 1 starts 8-byte aligned and no more
    d2 = torch.zeros((2, c.stride, 2), dtype=torch.float32, device="cuda")
    d2[0, :c.n[B.CLEAN_A]] = c.d_x[B.CLEAN_A, :c.n[B.CLEAN_A]]
    d2[1, 2:2 + c.n[s]] = c.d_x[s, :c.n[s]]
    assert (d2.data_ptr() + 8 * (c.stride + 2)) % 16 == 8
    ps = B.make_batch(2)
    got = B.run_batch(ps, d2, c.stride, [c.n[B.CLEAN_A], c.n[s]], {0: B.sizes_of(B.CLEAN_A), 1: B.sizes_of(s)}, first0=[0, 2])
    ps.close()
    assert got.calls[1] == want and got.calls[0] == B.single_reference(B.CLEAN_A, True)


# ------------------------------------------------------------------ 2. gather
def searched_whole():
    """a batch of five behind one search of every whole stream: (handle, the run)"""
    c = B.streams()
    ps = B.make_batch(5)
    return ps, B.run_batch(ps, c.d_x, c.stride, c.n)


def test_gather_slots_offsets_and_records():
    import torch
    c = B.streams()
    ps, run = searched_whole()
    sel = [B.selected(run.recs[s], c.n[s]) for s in range(5)]
    counts = [len(k) for k in sel]
    total = sum(counts)
    assert counts[B.CLEAN_A] == counts[B.CLEAN_B] == 5 and counts[B.NOISE_ONLY] == counts[B.EMPTY] == 0  # the lock comes with the second header
    g = B.gather(ps, c.d_x, c.stride, run.d_f, 5)
    assert g.offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert (g.tail == T.SENTINEL).all()
    i = 0
    for s in range(5):
        # the single-stream gather of the same stream: its frames back to back
        if counts[s]:
            one, single, d_f1 = B.run_single(c.d_x.data_ptr() + 8 * c.stride * s, c.n[s])
            d_out = B.zeros((counts[s] * FRAME_LEN + 90) * 2)
            d_cnt = B.zeros(1, "int32")
            single.gather_device(c.d_x.data_ptr() + 8 * c.stride * s, d_f1.data_ptr(), single.max_frames, PLSC, d_out.data_ptr(), d_cnt.data_ptr(), T.stream())
            torch.cuda.synchronize()
            assert int(d_cnt.item()) == counts[s]
            back = d_out.cpu().numpy().view(np.complex64)
            single.close()
        for k, f in enumerate(sel[s]):
            sof = int(run.recs[s][f]["sof_index"])
            assert bits(g.slots[i, :FRAME_LEN]) == bits(back[k * FRAME_LEN:(k + 1) * FRAME_LEN]), (s, f)
            assert bits(g.slots[i, FRAME_LEN:]) == bits(c.x[s, sof + FRAME_LEN:sof + FRAME_LEN + 90]), (s, f)
            assert g.slot_record[i].tolist() == [s, f]
            i += 1
    assert i == total and (g.slots[total:].view(np.uint32) == T.SENTINEL).all() and (g.slot_record[total:] == -7).all()
    # SEQ6 has a dummy frame behind data frames 2 and 4: the slot of such a frame ends in the DUMMY frame's header, not in the next data
    # frame's (which the back-to-back layout of the single-stream gather puts there)
    for s in (B.CLEAN_A, B.CLEAN_B):
        recs = run.recs[s]
        mixed = 0
        for k, f in enumerate(sel[s]):
            if f + 1 < len(recs) and recs[f + 1]["plsc"] == L.DUMMY:
                slot = g.slots[g.offsets[s] + k]
                dummy_sof, next_data = int(recs[f + 1]["sof_index"]), int(recs[sel[s][k + 1]]["sof_index"])
                assert dummy_sof == int(recs[f]["sof_index"]) + FRAME_LEN
                assert bits(slot[FRAME_LEN:]) == bits(c.x[s, dummy_sof:dummy_sof + 90]) != bits(c.x[s, next_data:next_data + 90])
                mixed += 1
        assert mixed == 2
    # a PLSC no stream carries, and no room at all: the offsets are still written, all zero
    d_off = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    ps.gather_device(c.d_x.data_ptr(), c.stride, run.d_f.data_ptr(), 5, P.plsc_of(4, 0, 1), g.d_slots.data_ptr(), 0, d_off.data_ptr(), 0, T.stream())
    torch.cuda.synchronize()
    assert d_off.cpu().tolist() == [0] * 6
    ps.close()


def test_gather_max_slots_below_the_total():
    c = B.streams()
    ps, run = searched_whole()
    full = B.gather(ps, c.d_x, c.stride, run.d_f, 5)
    total = int(full.offsets[-1])
    g = B.gather(ps, c.d_x, c.stride, run.d_f, 5, max_slots=total - 1, room=total - 1)
    assert g.offsets.tolist() == full.offsets.tolist()  # the true counts
    assert (g.tail == T.SENTINEL).all(), "the slot at max_slots was written"
    assert bits(g.slots) == bits(full.slots[:total - 1]) and bits(g.slot_record) == bits(full.slot_record[:total - 1])
    ps.close()


# ------------------------------------------------------------------ 3. coarse estimate
F_OFFSET = 2e-4  # cycles per symbol on stream CLEAN_B: inside the corrected range, so the flag changes at the first window's end


@pytest.mark.parametrize("period", [1, 3])
def test_coarse_estimate_equals_single_handles(period):
    """two searches per stream (the window state crosses a call per stream), each followed by gather and the batched estimate; per stream
    a single PlCoarse over the same slots in the same two calls gives the same bits"""
    import torch
    c = B.streams()
    d_x = c.d_x.clone()
    rot = Rotator(2.0 * np.pi * F_OFFSET)
    row = d_x.data_ptr() + 8 * c.stride * B.CLEAN_B
    rot.work_device(row, c.n[B.CLEAN_B], row, T.stream())
    torch.cuda.synchronize()
    rot.close()
    ps = B.make_batch(5)
    pcb = PlCoarseBatch(period, -1, max_streams=5, max_slots=32)
    singles = {s: PlCoarse(period, -1, max_frames=32) for s in SEQ_STREAMS}
    d_f = B.zeros(5 * ps.max_frames * 16, "uint8")
    d_plsc = torch.full((32,), PLSC, dtype=torch.uint8, device="cuda")
    pos = [0] * 5
    seen = {s: [] for s in SEQ_STREAMS}
    for call in range(2):
        n = [min(c.n[s] - pos[s], 34567 + 1000 * s) if call == 0 else c.n[s] - pos[s] for s in range(5)]
        n[B.EMPTY] = 0
        ps.work_device(d_x.data_ptr(), c.stride, pos, n, d_f.data_ptr(), T.stream())
        g = B.gather(ps, d_x, c.stride, d_f, 5, max_slots=32)  # no host read in between is needed: the counts are read for the checks only
        out = [B.zeros(32), B.zeros(32, "int32"), B.zeros(32, "int32")]
        for o in out:
            o.fill_(-5)
        pcb.work_device(g.d_slots.data_ptr(), SLOT, g.d_off.data_ptr(), 5, d_plsc.data_ptr(), *[o.data_ptr() for o in out], stream=T.stream())
        _, consumed, _ = ps.finish()
        pos = [pos[s] + int(consumed[s]) for s in range(5)]
        got = [o.cpu().numpy() for o in out]
        total = int(g.offsets[-1])
        assert all((a[total:] == -5).all() for a in got)
        for s in SEQ_STREAMS:
            a, b = int(g.offsets[s]), int(g.offsets[s + 1])
            assert b > a, "every SEQ6 stream has slots in both calls"
            ref = [B.zeros(b - a), B.zeros(b - a, "int32"), B.zeros(b - a, "int32")]
            singles[s].work_device(g.d_slots.data_ptr() + 8 * SLOT * a, SLOT, b - a, d_plsc.data_ptr(), *[o.data_ptr() for o in ref], stream=T.stream())
            torch.cuda.synchronize()
            for name, x, y in zip(("coarse_foffset", "coarse_corrected", "new_est"), got, ref):
                assert bits(x[a:b]) == bits(y.cpu().numpy()), f"stream {s}, call {call}: {name} {x[a:b]} against {y.cpu().numpy()} of the single handle"
            seen[s].append([x[a:b].copy() for x in got])
    for s in SEQ_STREAMS:
        fo, cc, ne = (np.concatenate([k[i] for k in seen[s]]) for i in range(3))
        print(f"period {period}, stream {s}: estimates {fo}, corrected {cc}, new_est {ne}")
        assert ne.sum() == len(ne) // period
    fo, cc, _ = (np.concatenate([k[i] for k in seen[B.CLEAN_B]]) for i in range(3))
    assert abs(fo[-1] - F_OFFSET) < 2e-5 and cc[-1] == 1
    if period == 3:
        assert cc.tolist()[:3] == [0, 0, 1]  # the flag changes within the run, and with it the form of the estimate
    assert abs(np.concatenate([k[0] for k in seen[B.CLEAN_A]])[-1]) < 2e-5
    # reset_stream: stream CLEAN_B's window starts again, the others' do not
    pcb.reset_stream(B.CLEAN_B)
    pcb.reset()
    for o in [ps, pcb, *singles.values()]:
        o.close()


# ------------------------------------------------------------------ 4. the strided front end
@pytest.mark.parametrize("pilots", [1, 0], ids=["pilots", "pilotless"])
def test_strided_front_end_equals_back_to_back(pilots):
    """an all-data sequence, so that the adjacent header of the back-to-back layout is the true next one: work_strided_device on the
    slots and work_device on the single-stream gather give the same XFECFRAMEs and the same estimates. The pilotless front end is the
    one that reads the next header."""
    import torch
    plsc, nd = P.plsc_of(1, 1, pilots), 5
    flen = M.pls_parse(plsc)["plframe_len"]
    _, d_x, n, _, _ = L.transmit_symbols([plsc] * nd, nd, B.GOLD, 901, 4200 + pilots, flush=0)
    rot = Rotator(2.0 * np.pi * 1e-5)  # a frequency offset the fine estimate has to find
    rot.work_device(d_x.data_ptr(), n, d_x.data_ptr(), T.stream())
    ps = B.make_batch(1)
    run = B.run_batch(ps, d_x, n, [n])
    cnt = nd - 1
    d_slots = B.zeros(cnt * (flen + 90) * 2)
    d_off = B.zeros(2, "int32")
    ps.gather_device(d_x.data_ptr(), n, run.d_f.data_ptr(), 1, plsc, d_slots.data_ptr(), cnt, d_off.data_ptr(), 0, T.stream())
    single = PlSync(plsc=-1, max_symbols=B.MAX_SYMBOLS, max_frames=B.MAX_FRAMES)
    d_f1, d_back, d_cnt = B.zeros(B.MAX_FRAMES * 16, "uint8"), B.zeros((cnt * flen + 90) * 2), B.zeros(1, "int32")
    single.work_device(d_x.data_ptr(), n, d_f1.data_ptr(), T.stream())
    single.gather_device(d_x.data_ptr(), d_f1.data_ptr(), B.MAX_FRAMES, plsc, d_back.data_ptr(), d_cnt.data_ptr(), T.stream())
    pc = PlCoarse(1, plsc, max_frames=cnt)
    d_fo, d_cc = B.zeros(cnt), B.zeros(cnt, "int32")
    pc.work_device(d_back.data_ptr(), flen, cnt, 0, d_fo.data_ptr(), d_cc.data_ptr(), 0, T.stream())
    torch.cuda.synchronize()
    assert d_off.cpu().tolist() == [0, cnt] and int(d_cnt.item()) == cnt and d_cc.cpu().tolist() == [1] * cnt
    fe = PlFrontEnd(B.GOLD, plsc, max_frames=cnt)

    def outputs():
        est = {k: B.zeros(cnt * (max(fe.n_pilots, 1) if k == "pilot_phase" else 1), np.dtype(dt).name) for k, dt in PlFrontEnd.EST}
        return B.zeros(cnt * fe.xfecframe_len * 2), est

    x0, e0 = outputs()
    x1, e1 = outputs()
    x2, e2 = outputs()
    fe.work_device(d_back.data_ptr(), cnt, 1, d_cc.data_ptr(), d_fo.data_ptr(), x0.data_ptr(), T.stream(), **{k: v.data_ptr() for k, v in e0.items()})
    fe.work_strided_device(d_slots.data_ptr(), flen + 90, cnt, d_cc.data_ptr(), d_fo.data_ptr(), x1.data_ptr(), T.stream(), **{k: v.data_ptr() for k, v in e1.items()})
    fe.estimate_strided_device(d_slots.data_ptr(), flen + 90, cnt, d_cc.data_ptr(), d_fo.data_ptr(), T.stream(), **{k: v.data_ptr() for k, v in e2.items()})
    torch.cuda.synchronize()
    assert bits(x0.cpu().numpy()) == bits(x1.cpu().numpy()) and x0.cpu().numpy().any() and not x2.cpu().numpy().any()
    for k in e0:
        assert bits(e0[k].cpu().numpy()) == bits(e1[k].cpu().numpy()) == bits(e2[k].cpu().numpy()), k
    fine = e1["fine_foffset"].cpu().numpy()
    print(f"{'pilots' if pilots else 'pilotless'}: fine offsets {fine}, valid {e1['fine_valid'].cpu().tolist()}")
    assert e1["fine_valid"].cpu().tolist() == [1] * cnt and (np.abs(fine - 1e-5) < 3e-6).all() and e1["plsc_decoded"].cpu().tolist() == [plsc] * cnt
    # a stride below plframe_len + 90 is refused, by the entry and by the host-only rule
    for entry, more in ((capi.lib.dvbs2_plframe_estimate_strided_device, ()), (capi.lib.dvbs2_plframe_process_strided_device, (x1.data_ptr(),))):
        T.refused(capi.EINVAL, "stride_syms below plframe_len + 90", entry, fe._h, d_slots.data_ptr(), flen + 89, cnt, d_cc.data_ptr(), d_fo.data_ptr(),
                  *more, None, None)
    for o in (fe, pc, single, ps, rot):
        o.close()


# ------------------------------------------------------------------ 5. end to end
def test_end_to_end_three_streams_in_one_pass():
    """samples of three SEQ6 streams -> batched SymbolSync -> PlSyncBatch -> gather -> PlCoarseBatch -> ONE strided front-end launch over all
    slots -> ONE FecChain call over all frames: every data frame of every stream comes back as that stream's encoder input, attributed
    through d_slot_record"""
    import torch
    st = T.stream()
    tx = [L.shaped_six_frames(lead, seed) for lead, seed in ((400, 5101), (733, 5102), (150, 5103))]
    ns = max(t.ns for t in tx)
    d_y = torch.zeros((3, ns, 2), dtype=torch.float32, device="cuda")
    for i, t in enumerate(tx):
        d_y[i, :t.ns] = t.d_y
    ss = SymbolSync(sps=L.SPS, loop_bw=0.01, damping=1.0, rolloff=L.ROLLOFF, interp_method=0, max_streams=3, max_samples=ns)
    d_sym = torch.zeros((3, ns, 2), dtype=torch.float32, device="cuda")
    ss.work_device(d_y.data_ptr(), ns, [t.ns for t in tx], d_sym.data_ptr(), ns, ns, 0, 0, st)
    n_out, _, status = ss.finish()  # (the symbol counts are host arrays of the search: the one host read in front of it)
    assert status.tolist() == [0, 0, 0] and all(abs(int(n_out[i]) - t.n_all) <= 12 for i, t in enumerate(tx))
    ps = PlSyncBatch(plsc=-1, max_streams=3, max_symbols=max(ns, PlSync.MIN_SYMBOLS), max_frames=16)
    pcb = PlCoarseBatch(1, PLSC, max_streams=3, max_slots=18)
    fe = PlFrontEnd(L.GOLD, PLSC, max_frames=18)
    d_f, d_slots, d_off, d_sr = B.zeros(3 * 16 * 16, "uint8"), B.zeros(18 * SLOT * 2), B.zeros(4, "int32"), B.zeros(36, "int32")
    d_fo, d_cc, d_rx = B.zeros(18), B.zeros(18, "int32"), B.zeros(18 * fe.xfecframe_len * 2)
    ps.work_device(d_sym.data_ptr(), ns, [0, 0, 0], n_out, d_f.data_ptr(), st)
    ps.gather_device(d_sym.data_ptr(), ns, d_f.data_ptr(), 3, PLSC, d_slots.data_ptr(), 18, d_off.data_ptr(), d_sr.data_ptr(), st)
    pcb.work_device(d_slots.data_ptr(), SLOT, d_off.data_ptr(), 3, 0, d_fo.data_ptr(), d_cc.data_ptr(), 0, st)
    # (the frame count of the launch is a host argument: 15 is what three SEQ6 streams give, checked against d_offsets below)
    total = 15
    fe.work_strided_device(d_slots.data_ptr(), SLOT, total, d_cc.data_ptr(), d_fo.data_ptr(), d_rx.data_ptr(), st)
    nf, _, state = ps.finish()
    torch.cuda.synchronize()
    offsets = d_off.cpu().tolist()
    assert offsets == [0, 5, 10, 15] and state.tolist() == [capi.PLSYNC_LOCKED] * 3 and d_cc.cpu().tolist()[:total] == [1] * total
    chain = FecChain(group_size=4, max_frames=total, max_trials=25, **L.QPSK_1_4_SHORT)
    chain.set_descramble(True)
    msg, ret, corr = chain.work(d_rx.cpu().numpy().view(np.complex64).reshape(18, -1)[:total], np.float32(0.02))
    chain.close()
    assert (ret >= 0).all() and (corr >= 0).all()
    recs, sr = B.records(d_f, 3, 16), d_sr.cpu().numpy().reshape(18, 2)
    seen = set()
    for i in range(total):
        s, f = (int(v) for v in sr[i])
        assert offsets[s] <= i < offsets[s + 1] and f < nf[s] and recs[s, f]["plsc"] == PLSC and recs[s, f]["flags"] & capi.PLSYNC_FLAG_LOCKED
        k = int(np.count_nonzero(recs[s, :f]["plsc"] == PLSC))  # which data frame of its stream the slot carries
        assert bits(msg[i]) == bits(tx[s].sent[k]), f"slot {i}: stream {s}, record {f}, data frame {k}"
        seen.add((s, k))
    assert seen == {(s, k) for s in range(3) for k in range(1, 6)}  # every data frame behind the lock of every stream
    for o in (fe, pcb, ps, ss):
        o.close()


# ------------------------------------------------------------------ 6. arguments
def test_arguments_on_a_live_handle():
    import torch
    lib = capi.lib
    c = B.streams()
    ps = B.make_batch(2, max_symbols=PlSync.MIN_SYMBOLS)
    d_f, d_off = B.zeros(2 * 16 * 16, "uint8"), B.zeros(3, "int32")
    two = np.array([10, 10], np.int32)
    zero = np.zeros(2, np.int32)
    p, x = two.ctypes.data, c.d_x.data_ptr()
    search = lib.dvbs2_plsync_batch_search_device
    T.refused(capi.ESIZE, "n_streams exceeds max_streams", search, ps._h, x, c.stride, zero.ctypes.data, p, 3, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "n_streams is negative", search, ps._h, x, c.stride, zero.ctypes.data, p, -1, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "first is null", search, ps._h, x, c.stride, None, p, 2, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "n_syms is null", search, ps._h, x, c.stride, zero.ctypes.data, None, 2, d_f.data_ptr(), None)
    big = np.array([10, PlSync.MIN_SYMBOLS + 1], np.int32)
    T.refused(capi.ESIZE, "n_syms[1] exceeds max_symbols", search, ps._h, x, c.stride, zero.ctypes.data, big.ctypes.data, 2, d_f.data_ptr(), None)
    neg = np.array([0, -1], np.int32)
    T.refused(capi.EINVAL, "first[1] is negative", search, ps._h, x, c.stride, neg.ctypes.data, p, 2, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "n_syms[1] is negative", search, ps._h, x, c.stride, zero.ctypes.data, neg.ctypes.data, 2, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "first[0] + n_syms[0] exceeds stride_syms", search, ps._h, x, 9, zero.ctypes.data, p, 2, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "bad argument", search, ps._h, None, c.stride, zero.ctypes.data, p, 2, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "bad argument", search, ps._h, x, c.stride, zero.ctypes.data, p, 2, None, None)
    T.refused(capi.EINVAL, "d_syms must be 8-byte aligned", search, ps._h, x + 4, c.stride, zero.ctypes.data, p, 2, d_f.data_ptr(), None)
    T.refused(capi.EINVAL, "stream index out of range", lib.dvbs2_plsync_batch_reset_stream, ps._h, 2)
    T.refused(capi.EINVAL, "stream index out of range", lib.dvbs2_plsync_batch_reset_stream, ps._h, -1)
    gather = lib.dvbs2_plsync_batch_gather_device
    d_s = B.zeros(SLOT * 2)
    T.refused(capi.EINVAL, "n_streams exceeds the streams of the last search", gather, ps._h, x, c.stride, d_f.data_ptr(), 1, PLSC, d_s.data_ptr(), 1, d_off.data_ptr(), None, None)
    T.refused(capi.EINVAL, "plsc out of range (0..127)", gather, ps._h, x, c.stride, d_f.data_ptr(), 1, 128, d_s.data_ptr(), 1, d_off.data_ptr(), None, None)
    T.refused(capi.EINVAL, "bad argument", gather, ps._h, x, c.stride, d_f.data_ptr(), 1, PLSC, d_s.data_ptr(), 1, None, None, None)
    T.refused(capi.ESIZE, "n_streams exceeds max_streams", gather, ps._h, x, c.stride, d_f.data_ptr(), 3, PLSC, d_s.data_ptr(), 1, d_off.data_ptr(), None, None)
    # an empty batch and a batch of empty streams are no-ops that report nothing
    ps.work_device(x, c.stride, [0, 0], [0, 0], d_f.data_ptr(), T.stream())
    nf, consumed, state = ps.finish()
    assert nf.tolist() == consumed.tolist() == state.tolist() == [0, 0]
    ps.gather_device(x, c.stride, d_f.data_ptr(), 2, PLSC, d_s.data_ptr(), 1, d_off.data_ptr(), 0, T.stream())
    torch.cuda.synchronize()
    assert d_off.cpu().tolist() == [0, 0, 0]
    pcb = PlCoarseBatch(1, -1, max_streams=2, max_slots=4)
    est = lib.dvbs2_plcoarse_batch_estimate_device
    T.refused(capi.EINVAL, "a handle without a fixed PLSC needs the per-slot PLSC array", est, pcb._h, d_s.data_ptr(), SLOT, None, d_off.data_ptr(), 2, None, None, None, None)
    T.refused(capi.EINVAL, "stride below the 90 header symbols", est, pcb._h, d_s.data_ptr(), 89, d_f.data_ptr(), d_off.data_ptr(), 2, None, None, None, None)
    T.refused(capi.ESIZE, "n_streams exceeds max_streams", est, pcb._h, d_s.data_ptr(), SLOT, d_f.data_ptr(), d_off.data_ptr(), 3, None, None, None, None)
    T.refused(capi.EINVAL, "bad argument", est, pcb._h, d_s.data_ptr(), SLOT, d_f.data_ptr(), None, 2, None, None, None, None)
    T.refused(capi.EINVAL, "stream index out of range", lib.dvbs2_plcoarse_batch_reset_stream, pcb._h, 2)
    h = C.c_void_p()
    for create, args in ((lib.dvbs2_plsync_batch_create, (-1, 3, 2, PlSync.MIN_SYMBOLS, 16)), (lib.dvbs2_plcoarse_batch_create, (1, -1, 2, 4))):
        h.value = 1
        T.refused(capi.EINVAL, "device index out of range", create, C.byref(h), *args, 99)  # good arguments, no such device
        assert not h.value
    pcb.close()
    ps.close()
