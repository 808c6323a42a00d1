"""PLFRAME search on the device (dvbs2_plsync_*) against the float64 model of tests/plsync_model.py: the timing metric within
the per-value bound the model derives from the float32 format, the tracker's records EXACTLY (index, PLSC, flags; the metric
within its bound), the gather step bit for bit, and unaligned noisy streams end to end into the FEC chain. Every stream is
vouched for by tests/test_plsync_model.py::test_guard_no_stream_is_excused: none of the model's decisions lies within
rounding of a threshold or a tie, so nothing is excused here. The metric is UNPINNED against the genuine reference (VOLK is
not part of the reference tree)."""
import ctypes as C

import numpy as np
import pytest

import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import FecChain, PlFrontEnd, PlSync, capi

pytestmark = pytest.mark.gpu

MAX_FRAMES = 8192


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def device_metric(ps, x):
    import torch
    d_x = dev(x) if x.size else torch.zeros(2, device="cuda")
    d_m = torch.full((max(x.size, 1),), -1.0, dtype=torch.float32, device="cuda")
    ps.metric_device(d_x.data_ptr(), x.size, d_m.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_m.cpu().numpy()[:x.size]


def device_search(ps, x, keep=False):
    """one work_device() + finish(); returns (records, consumed, state[, device tensors])"""
    import torch
    d_x = dev(x) if x.size else torch.zeros(2, device="cuda")
    d_f = torch.zeros(ps.max_frames * 16, dtype=torch.uint8, device="cuda")
    ps.work_device(d_x.data_ptr(), x.size, d_f.data_ptr(), torch.cuda.current_stream().cuda_stream)
    nf, consumed, state = ps.finish()
    recs = d_f.cpu().numpy().view(PlSync.FRAME_DTYPE)[:nf].copy()
    return (recs, consumed, state, d_x, d_f) if keep else (recs, consumed, state)


def extra(name):
    """a stream of P.extra_cases(): covered by the guard test like every other"""
    return P.build_case(*next(c for c in P.extra_cases() if c[0] == name))


def make_sync(trk, max_symbols, max_frames=MAX_FRAMES):
    return PlSync(plsc=trk.get("fixed_plsc", -1), unlock_thresh=trk.get("unlock_thresh", 3), max_symbols=max(max_symbols, PlSync.MIN_SYMBOLS),
                  max_frames=max_frames, coherent=trk.get("coherent", 1), soft=trk.get("soft", 1), expected_pls=trk.get("enabled"))


def compare_records(got, c, what, base=0):
    want = c["recs"]
    print(f"{what}: {len(got)} records on the device, {len(want)} in the model, "
          f"{sum(1 for r in want if r[3] & 2)} locked, {sum(1 for r in want if not r[3] & 1)} inferred")
    assert len(got) == len(want)
    assert got["sof_index"].tolist() == [r[0] + base for r in want]
    assert got["plsc"].tolist() == [r[2] for r in want]
    assert got["flags"].tolist() == [r[3] for r in want]
    if len(want):
        n = np.array([r[0] + 89 for r in want])
        err = np.abs(got["metric"].astype(np.float64) - np.array([r[1] for r in want]))
        print(f"{what}: metric worst error / bound {np.max(err / c['bound'][n]):.3f}")
        assert (err <= c["bound"][n]).all()


# ------------------------------------------------------------------ 1. the timing metric
def test_metric_against_the_model():
    x = extra("metric-stream")["x"]  # amplitude 0.8, not unit energy: the bound scales with the symbols
    ps = PlSync(max_symbols=max(x.size, PlSync.MIN_SYMBOLS), max_frames=16)
    # zero history: the whole stream (longer than several tiles), and buffers of 1, 89, 90 and 91 symbols
    want, bound = P.metric(x)
    for n in (x.size, 1, 89, 90, 91, 1792, 1793):
        got = device_metric(ps, x[:n])
        err = np.abs(got - want[:n])
        print(f"metric, {n} symbols, zero history: worst error / bound {np.max(err / bound[:n]):.3f}, largest value {got.max():.2f}")
        assert (err <= bound[:n]).all()
    whole = device_metric(ps, x)
    assert whole.max() > 57.0 * 0.64 * 0.8 and (whole >= 0).all()  # the peaks: 57 |x|^2, less what the noise takes
    # carried history: the stream in three calls cut at arbitrary points; searching consumes every symbol of a call that ends
    # before any frame is complete, so the handle's history is the 89 symbols before each cut
    cuts = [0, 517, 1100, x.size]  # the first header ends at index 1323
    ps.reset()
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        hist = np.concatenate([np.zeros(P.HIST, np.complex64), x[:a]])[-P.HIST:]
        got = device_metric(ps, x[a:b])
        w, bd = P.metric(x[a:b], hist)
        assert (np.abs(got - w) <= bd).all()
        parts.append(got)
        if b < x.size:
            _, consumed, _ = device_search(ps, x[a:b])  # advances the handle: no frame fits into these short calls
            assert consumed == b - a
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))  # the same bits wherever the cut falls
    # a long buffer
    big = np.tile(x, 1 + (1 << 20) // x.size)[:(1 << 20) + 3]
    pb = PlSync(max_symbols=big.size, max_frames=16)
    got = device_metric(pb, big)
    w, bd = P.metric(big)
    print(f"metric, {big.size} symbols: worst error / bound {np.max(np.abs(got - w) / bd):.3f}")
    assert (np.abs(got - w) <= bd).all()
    pb.close()
    ps.close()


# ------------------------------------------------------------------ 2. the tracker, one call per stream
@pytest.mark.parametrize("name,stream,trk", P.cases(), ids=[c[0] for c in P.cases()])
def test_search_records_equal_the_model(name, stream, trk):
    c = P.build_case(name, stream, trk)
    ps = make_sync(trk, c["x"].size)
    got, consumed, state = device_search(ps, c["x"])
    compare_records(got, c, name)
    assert (consumed, state) == (c["consumed"], c["state"])
    # the host entry gives the same records
    ps.reset()
    hrecs, hcons, hstate = ps.work(c["x"])
    assert hrecs.tobytes() == got.tobytes() and (hcons, hstate) == (consumed, state)
    ps.close()


# ------------------------------------------------------------------ 3. the same streams in calls of awkward sizes
CHUNKED = ["acm-11", "acm-00", "acm-3dB", "removed-1", "removed-2", "removed-3-fixed", "ccm-16-3-decode", "ccm-17-0-fixed", "ccm-72-0-decode",
           "ccm-97-10-decode", "ccm-0-3-decode", "ccm-55-clean-fixed"]
SIZES = (33461, 35003, 39999, 34567)  # each at least 89 + 33282 + 90: a pending frame always fits into the next call


def run_chunked(ps, x, sizes=SIZES, tiny=()):
    """follow `consumed` through x; after every call that left a frame pending, first present calls of `tiny` symbols from the
    pending SOF: shorter than a PLHEADER, they must consume and report nothing and leave the machine where it was"""
    recs, pos, i, calls = [], 0, 0, 0
    while True:
        n = min(sizes[i % len(sizes)], x.size - pos)
        r, consumed, state = device_search(ps, x[pos:pos + n])
        if consumed < n:
            for t in tiny:
                rt, ct, st = device_search(ps, x[pos + consumed:pos + consumed + t])
                assert (len(rt), ct, st) == (0, 0, state)
        recs.append(r)
        calls += 1
        at_end = pos + n == x.size
        pos += consumed
        i += 1
        assert 0 <= consumed <= n and calls < 10000
        if at_end:
            return np.concatenate(recs), pos, state, calls
        assert consumed > 0


@pytest.mark.parametrize("tiny", [(), (1, 89, 50)], ids=["plain", "tiny-calls-after-pending"])
@pytest.mark.parametrize("name", CHUNKED)
def test_search_in_awkward_calls_equals_one_call(name, tiny):
    name, stream, trk = next(c for c in P.cases() if c[0] == name)
    c = P.build_case(name, stream, trk)
    ps = make_sync(trk, max(SIZES))
    got, pos, state, calls = run_chunked(ps, c["x"], tiny=tiny)
    compare_records(got, c, f"{name} in {calls} calls")
    assert state == c["state"] and pos == c["consumed"]
    ps.close()


def test_max_frames_overflow_and_reset():
    name, stream, trk = next(c for c in P.cases() if c[0] == "acm-11")
    c = P.build_case(name, stream, trk)
    x = c["x"]
    ps = make_sync(trk, x.size, max_frames=3)
    got, consumed, state = device_search(ps, x)
    assert len(got) == 3 and consumed == c["recs"][3][0]  # stops at the fourth frame's SOF
    assert got["sof_index"].tolist() == [r[0] for r in c["recs"][:3]]
    # following `consumed` gives every record once
    recs, pos = [got], consumed
    for _ in range(20):
        r, consumed, state = device_search(ps, x[pos:])
        recs.append(r)
        pos += consumed
        if len(r) < 3:
            break
    compare_records(np.concatenate(recs), c, "acm-11 with max_frames 3")
    assert state == c["state"]
    # reset: the block as constructed, indices count from zero again
    ps.reset()
    again, _, _ = device_search(ps, x)
    assert again.tobytes() == got.tobytes()
    ps.close()


# ------------------------------------------------------------------ 4. gather, and into the front end
def gather(ps, d_x, d_f, n_frames, wanted, capacity_syms):
    import torch
    d_out = torch.zeros(capacity_syms * 2, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ps.gather_device(d_x.data_ptr(), d_f.data_ptr(), n_frames, wanted, d_out.data_ptr(), d_cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out, int(d_cnt.item())


@pytest.mark.parametrize("offset", [700, 701])  # an even and an odd start: aligned and unaligned 16-byte loads
def test_gather_equals_slicing_and_feeds_the_front_end(offset):
    c = extra(f"gather-{offset}")
    x, sofs = c["x"], c["sofs"]
    ps = PlSync(max_symbols=x.size, max_frames=64)
    recs, consumed, state, d_x, d_f = device_search(ps, x, keep=True)
    compare_records(recs, c, f"gather-{offset}")
    assert recs["sof_index"].tolist() == sofs and recs["plsc"].tolist() == P.ACM_PLSCS and state == capi.PLSYNC_LOCKED
    for wanted in (P.SHORT_QPSK, P.plsc_of(0, 0, 0), P.plsc_of(13, 0, 0), P.plsc_of(24, 0, 1)):
        L = M.pls_parse(wanted)["plframe_len"]
        sel = [int(r["sof_index"]) for r in recs if r["flags"] & 2 and r["plsc"] == wanted]
        d_out, cnt = gather(ps, d_x, d_f, ps.max_frames, wanted, len(sel) * L + 90 + 8)
        assert cnt == len(sel)
        if not sel:
            continue
        want = np.concatenate([x[s:s + L] for s in sel] + [x[sel[-1] + L:sel[-1] + L + 90]])
        got = d_out.cpu().numpy().view(np.complex64)
        assert np.array_equal(got[:want.size].view(np.uint32), want.view(np.uint32)) and not got[want.size:].any()
        # the gathered layout through PlFrontEnd = PlFrontEnd on the frames as the transmitter aligned them
        if wanted == P.SHORT_QPSK:
            import torch
            fe = PlFrontEnd(5, wanted, max_frames=cnt)
            cc = torch.ones(cnt, dtype=torch.int32, device="cuda")
            d_o = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
            d_p = torch.zeros(cnt, dtype=torch.uint8, device="cuda")
            fe.work_device(d_out.data_ptr(), cnt, 1, cc.data_ptr(), 0, d_o.data_ptr(), 0, plsc_decoded=d_p.data_ptr())
            torch.cuda.synchronize()
            aligned = np.stack([x[s:s + L] for s in sel])
            ref, est = fe.work(aligned, np.ones(cnt, np.int32), trailing_header=x[sel[-1] + L:sel[-1] + L + 90].copy())
            assert np.array_equal(d_o.cpu().numpy().view(np.uint32), ref.view(np.uint32))
            assert d_p.cpu().tolist() == est["plsc_decoded"].tolist() == [wanted] * cnt  # the tracker's decoder is the front end's
            fe.close()
    # records that are not locked (the first header) are never gathered; n_frames = 0 gives a count of 0
    first = int(recs["plsc"][0])
    assert not recs["flags"][0] & 2
    _, cnt = gather(ps, d_x, d_f, 1, first, M.pls_parse(first)["plframe_len"] + 98)
    assert cnt == 0
    _, cnt = gather(ps, d_x, d_f, 0, first, 98)
    assert cnt == 0
    ps.close()


# ------------------------------------------------------------------ 5. end to end: unaligned noisy stream -> BBFRAME bytes
@pytest.mark.parametrize("name,constellation", [("e2e-qpsk", capi.MOD_QPSK), ("e2e-8psk", capi.MOD_8PSK)])
def test_end_to_end_from_an_unaligned_stream(name, constellation):
    import torch
    e, nf, gold = P.E2E[name], P.E2E_FRAMES, P.E2E_GOLD
    short, rate, es_n0_db = e["short"], e["rate"], e["es_n0_db"]
    plsc = P.plsc_of(e["modcod"], short, 1)
    framesize = capi.FECFRAME_SHORT if short else capi.FECFRAME_NORMAL
    c = extra(name)
    x, sofs, sent = c["x"], c["sofs"], c["sent"]
    L = M.pls_parse(plsc)["plframe_len"]
    ps = PlSync(max_symbols=x.size, max_frames=64)
    recs, consumed, state, d_x, d_f = device_search(ps, x, keep=True)
    compare_records(recs, c, name)
    # at these Es/N0 the threshold of 30 is also crossed inside frames (false detections while `found`, as in the reference);
    # what counts is every frame the tracker reports as locked with this PLSC: each must be a transmitted frame, intact
    locked = [int(r["sof_index"]) for r in recs if r["flags"] & 2 and r["plsc"] == plsc]
    print(f"{len(recs)} records, {len(locked)} locked frames of PLSC {plsc}, final state {state}")
    assert state == capi.PLSYNC_LOCKED and len(locked) >= nf // 2 and set(locked) <= set(sofs)
    which = [sofs.index(s) for s in locked]
    d_fr, cnt = gather(ps, d_x, d_f, len(recs), plsc, len(locked) * L + 90)
    assert cnt == len(locked)
    fe = PlFrontEnd(gold, plsc, max_frames=cnt)
    cc = torch.ones(cnt, dtype=torch.int32, device="cuda")
    d_xfec = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
    fe.work_device(d_fr.data_ptr(), cnt, 1, cc.data_ptr(), 0, d_xfec.data_ptr(), 0)
    torch.cuda.synchronize()
    chain = FecChain(framesize=framesize, rate=rate, constellation=constellation, group_size=4, max_frames=cnt, max_trials=25)
    msg, ret, corr = chain.work(d_xfec.cpu().numpy().view(np.complex64), np.float32(10 ** (-es_n0_db / 10)))
    assert (ret >= 0).all() and (corr >= 0).all()
    assert np.array_equal(msg, sent[which])
    chain.close()
    fe.close()
    ps.close()


# ------------------------------------------------------------------ 6. arguments
def test_arguments():
    import torch
    lib, h = capi.lib, C.c_void_p()
    ok = PlSync.MIN_SYMBOLS
    for plsc, ut, ms, mf in ((-1, 3, ok - 1, 16), (128, 3, ok, 16), (-2, 3, ok, 16), (-1, 0, ok, 16), (-1, 256, ok, 16), (-1, 3, ok, 0)):
        assert lib.dvbs2_plsync_create(C.byref(h), plsc, ut, ms, mf, 0) == capi.EINVAL and not h.value
        assert lib.dvbs2_last_error()
    assert lib.dvbs2_plsync_create(C.byref(h), -1, 3, 100, 16, 0) == capi.EINVAL and b"33282" in lib.dvbs2_last_error()
    ps = PlSync(max_symbols=ok, max_frames=4)
    d = torch.zeros(2 * (ok + 1), device="cuda")
    f = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib.dvbs2_plsync_search_device(ps._h, d.data_ptr(), ok + 1, f.data_ptr(), None) == capi.ESIZE and b"max_symbols" in lib.dvbs2_last_error()
    assert lib.dvbs2_plsync_search_device(ps._h, None, 10, f.data_ptr(), None) == capi.EINVAL
    assert lib.dvbs2_plsync_search_device(ps._h, d.data_ptr(), 10, None, None) == capi.EINVAL
    assert lib.dvbs2_plsync_search_device(ps._h, d.data_ptr(), -1, f.data_ptr(), None) == capi.EINVAL
    assert lib.dvbs2_plsync_metric_device(ps._h, d.data_ptr(), 10, None, None) == capi.EINVAL
    assert lib.dvbs2_plsync_gather_device(ps._h, d.data_ptr(), f.data_ptr(), 5, 4, d.data_ptr(), cnt.data_ptr(), None) == capi.ESIZE
    assert lib.dvbs2_plsync_gather_device(ps._h, d.data_ptr(), f.data_ptr(), 4, 128, d.data_ptr(), cnt.data_ptr(), None) == capi.EINVAL
    assert lib.dvbs2_plsync_gather_device(ps._h, d.data_ptr(), f.data_ptr(), 4, 4, d.data_ptr(), None, None) == capi.EINVAL
    bad = np.array([0, 128], np.uint8)
    assert lib.dvbs2_plsync_set_expected_pls(ps._h, bad.ctypes.data, 2) == capi.EINVAL and b"128" in lib.dvbs2_last_error()
    assert lib.dvbs2_plsync_set_expected_pls(ps._h, None, 2) == capi.EINVAL
    with pytest.raises(TypeError):
        ps.work(np.zeros(10, np.complex128))
    with pytest.raises(ValueError):
        ps.work(np.zeros(ok + 1, np.complex64))
    # an empty call is a no-op that reports nothing; zeros never lock
    recs, consumed, state = ps.work(np.zeros(0, np.complex64))
    assert len(recs) == 0 and consumed == 0 and state == capi.PLSYNC_SEARCHING
    recs, consumed, state = ps.work(np.zeros(5000, np.complex64))
    assert len(recs) == 0 and consumed == 5000 and state == capi.PLSYNC_SEARCHING
    ps.close()
