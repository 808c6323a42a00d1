"""GPU: the de-header rows (include/dvbs2_fec_hip.h, "de-header rows"; notes/bbdeheader_rows.md) -- S streams de-headed in five launches
from records in device memory, the frame ranges read from d_offsets on the device.
  1. five streams in one call against the model (tests/bbdeheader_rows_model.py: one OracleBbDeheader per stream) and against a single
     BbDeheader handle per stream, byte for byte;
  2. the same streams in calls cut at other points per stream;
  3. the other frame sizes;
  4. max_frames below the frame count, a pair of offsets that decreases, the reset of one record;
  5. end to end: three carriers from samples to TS packets, d_offsets never read by the host.
kbch 3072 (a DATAFIELD of 374 bytes) makes nearly every frame carry a straddling head; 300 frames are more than one frame per scan
thread; the one-frame and the empty stream are the edges of the scan's chunks."""
import ctypes as C
import functools

import numpy as np
import pytest

import bbdeheader_rows_model as BM
import fec_testlib as T
import loopback as L
from dvbs2rx_amd import (BBDEHEADER_STATE, BbDeheader, BbFramer, FecChain, FecEncoder, PlCoarseBatch, PlFramer, PlFrontEnd, PlSync, PlSyncBatch,
                         PulseShaper, SymbolSync, bbdeheader_rows_device, bbdeheader_rows_geometry, bbdeheader_state_counters, capi,
                         plframer_layout, pulse_geometry)

pytestmark = pytest.mark.gpu

KBCH = 3072
FUZZ_SEED = 41
GUARD, FILL = 4096, 0xA5
PATTERN = np.arange(256, dtype=np.uint8) ^ 0x5A  # a record no call must touch


@functools.lru_cache(None)
def five_streams():
    """healthy 300, fuzzed 300, all headers bad, empty, healthy 1"""
    fuzz = BM.fuzzed(KBCH, 320, FUZZ_SEED)
    assert len(fuzz) >= 300
    fr = [BM.healthy(KBCH, 300, 1)[1], fuzz[:300], BM.bad_headers(KBCH, 7, 3), np.zeros((0, KBCH // 8), np.uint8), BM.healthy(KBCH, 1, 5)[1]]
    for f in fr:
        f.setflags(write=False)
    return fr


@functools.lru_cache(None)
def five_streams_one_call():
    """the model's (TS bytes per stream, pkt_offsets, records, counters) of five_streams() in one call"""
    m = BM.Rows(KBCH, 5)
    out, pko = m.call(five_streams())
    return out, pko, m.records(), m.counters()


class Rows:
    """the device buffers of n_streams streams with max_frames: the records between two guard records, guard bytes behind d_ts_out and
    behind d_pkt_offsets; call() checks them all"""

    def __init__(self, kbch, n_streams, max_frames):
        import torch
        self.kbch, self.S, self.max_frames = kbch, n_streams, max_frames
        self.g = bbdeheader_rows_geometry(kbch, n_streams, max_frames)
        self.state = torch.full(((n_streams + 2) * 256,), FILL, dtype=torch.uint8, device="cuda")
        self.state[256:-256] = 0
        self.work = torch.zeros(self.g["work_bytes"], dtype=torch.uint8, device="cuda")
        self.out = torch.zeros(self.g["out_bytes"] + GUARD, dtype=torch.uint8, device="cuda")
        self.pko = torch.zeros(n_streams + 1 + 8, dtype=torch.int32, device="cuda")
        assert self.state.data_ptr() % 16 == 0 and self.work.data_ptr() % 16 == 0

    def state_ptr(self, s=0):
        return self.state.data_ptr() + 256 * (1 + s)

    def set_record(self, s, record_bytes):
        import torch
        self.state[256 * (1 + s):256 * (2 + s)] = torch.from_numpy(np.array(record_bytes, np.uint8)).cuda()

    def records(self):
        st = self.state.cpu().numpy()
        assert (st[:256] == FILL).all() and (st[-256:] == FILL).all(), "a write around the records"
        return st[256:-256].view(BBDEHEADER_STATE).copy()

    def call(self, frames, offsets=None, stream=None):
        """frames[s]: the BBFRAMEs of stream s, packed stream-major; offsets overrides the packed ones. Returns (TS bytes per stream,
        pkt_offsets)."""
        import torch
        bb, off = BM.pack(frames, self.kbch // 8)
        if offsets is not None:
            off = np.array(offsets, np.int32)
        d_bb = torch.from_numpy(np.concatenate([bb, np.zeros((1, self.kbch // 8), np.uint8)])).cuda()
        d_off = torch.from_numpy(off).cuda()
        self.out.fill_(FILL)
        self.pko.fill_(-7)
        bbdeheader_rows_device(d_bb.data_ptr(), self.kbch, d_off.data_ptr(), self.S, self.max_frames, self.state_ptr(), self.work.data_ptr(),
                               self.g["work_bytes"], self.out.data_ptr(), self.g["out_bytes"], self.pko.data_ptr(), 0, T.stream() if stream is None else stream)
        torch.cuda.synchronize()
        pko, out = self.pko.cpu().numpy(), self.out.cpu().numpy()
        assert (pko[self.S + 1:] == -7).all(), "a write behind pkt_offsets"
        assert pko[0] == 0 and (np.diff(pko[:self.S + 1]) >= 0).all()
        assert (out[int(pko[self.S]) * 188:] == FILL).all(), "a write behind the packets of the call"
        return [out[int(a) * 188:int(b) * 188].copy() for a, b in zip(pko[:self.S], pko[1:self.S + 1])], pko[:self.S + 1].tolist()


def same_stream(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    assert np.array_equal(got, want), f"{what}: the first differing byte at {np.flatnonzero(got != want)[0]}"


# ------------------------------------------------------------------ 1. five streams in one call
def test_the_fuzz_seed_meets_everything():
    """asserted on the CPU from the oracle alone: the fuzzed stream has dropped frames, gaps, overruns and packet errors and still gives
    more than half the packets of the healthy one"""
    _, _, _, counters = five_streams_one_call()
    c = counters[1]
    assert c["dropped"] > 0 and c["gaps"] > 0 and c["overruns"] > 0 and c["errors"] > 0 and c["packets"] > counters[0]["packets"] // 2
    assert counters[0]["packets"] == 300 * 374 // 188 and counters[2]["dropped"] == 7 and counters[2]["packets"] == 0 and counters[4]["packets"] == 1


def test_five_streams_in_one_call():
    frames = five_streams()
    want, want_pko, want_rec, want_counters = five_streams_one_call()
    rows = Rows(KBCH, 5, 700)
    rows.set_record(3, PATTERN)
    got, pko = rows.call(frames)
    assert pko == want_pko
    for s in range(5):
        same_stream(got[s], want[s], f"stream {s} against the oracle")
    rec = rows.records()
    assert rec[3].tobytes() == PATTERN.tobytes(), "the empty stream's record was touched"
    for s in (0, 1, 2, 4):
        assert rec[s].tobytes() == want_rec[s].tobytes(), f"record {s}: {rec[s]} != {want_rec[s]}"
    assert [c for s, c in enumerate(bbdeheader_state_counters(rec)) if s != 3] == [c for s, c in enumerate(want_counters) if s != 3]
    # the single handle fed the same frames
    for s in (0, 1, 2, 4):
        one = BbDeheader(kbch_bits=KBCH, max_frames=300)
        same_stream(got[s], one.work(frames[s]), f"stream {s} against a single handle")
        assert one.counters() == bbdeheader_state_counters(rec[s:s + 1])[0], s
        one.close()


# ------------------------------------------------------------------ 2. calls cut at other points per stream
CUTS = ([0, 1, 8, 40, 300], [0, 0, 7, 39, 300], [0, 3, 3, 7, 7], [0, 0, 0, 0, 0], [0, 0, 0, 1, 1])  # per stream: frames presented so far, per call


def test_cut_calls_give_the_bytes_of_one_call():
    """four calls; every stream is cut elsewhere, streams 1, 2 and 4 get no frame in some calls: per call the model's bytes, a record
    without frames keeps its bytes, and behind the last call packets and records are those of one call"""
    frames = five_streams()
    whole, _, whole_rec, _ = five_streams_one_call()
    rows, model = Rows(KBCH, 5, 700), BM.Rows(KBCH, 5)
    parts = [[] for _ in range(5)]
    for k in range(4):
        piece = [frames[s][CUTS[s][k]:CUTS[s][k + 1]] for s in range(5)]
        before = rows.records()
        got, pko = rows.call(piece)
        want, want_pko = model.call(piece)
        assert pko == want_pko, k
        after = rows.records()
        for s in range(5):
            same_stream(got[s], want[s], f"call {k}, stream {s}")
            parts[s].append(got[s])
            if len(piece[s]) == 0:
                assert after[s].tobytes() == before[s].tobytes(), f"call {k}: stream {s} got no frame and its record changed"
        assert BM.canon(after).tobytes() == BM.canon(model.records()).tobytes(), k
    for s in range(5):
        same_stream(np.concatenate(parts[s]), whole[s], f"stream {s}: the calls together")
    assert BM.canon(rows.records(), last_packets=False).tobytes() == BM.canon(whole_rec, last_packets=False).tobytes()


# ------------------------------------------------------------------ 3. the other frame sizes
@pytest.mark.parametrize("kbch", [16008, 58192])
def test_other_frame_sizes(kbch):
    """3 healthy streams of 4 frames; kbch 58192 completes up to 39 packets per frame"""
    streams = [BM.healthy(kbch, 4, 10 + s) for s in range(3)]
    rows, model = Rows(kbch, 3, 12), BM.Rows(kbch, 3)
    assert rows.g["max_out_bytes_per_frame"] == {16008: 11, 58192: 39}[kbch] * 188
    got, pko = rows.call([fr for _, fr in streams])
    want, want_pko = model.call([fr for _, fr in streams])
    assert pko == want_pko
    for s, (ups, _) in enumerate(streams):
        same_stream(got[s], want[s], f"stream {s}")
        same_stream(got[s], ups[:4 * ((kbch - 80) // 8) // 188 * 188], f"stream {s}: the user packets")
    assert rows.records().tobytes() == model.records().tobytes()


# ------------------------------------------------------------------ 4. clipping, a decreasing pair, the reset
def three_streams():
    return [BM.healthy(KBCH, 5, 21)[1], BM.fuzzed(KBCH, 12, 22)[:4], BM.healthy(KBCH, 6, 23)[1]]


def test_max_frames_one_below_the_frame_count():
    """15 frames with max_frames 14: the last frame of the last stream is ignored; presented in the next call it gives the bytes of one
    call. Every buffer has the geometry's size for 14 frames."""
    frames = three_streams()
    assert [len(f) for f in frames] == [5, 4, 6]
    rows, model, whole = Rows(KBCH, 3, 14), BM.Rows(KBCH, 3), BM.Rows(KBCH, 3)
    want_whole, _ = whole.call(frames)
    got1, pko1 = rows.call(frames)  # offsets [0, 5, 9, 15]
    want1, want_pko1 = model.call([frames[0], frames[1], frames[2][:5]])
    assert pko1 == want_pko1
    for s in range(3):
        same_stream(got1[s], want1[s], f"clipped call, stream {s}")
    assert rows.records().tobytes() == model.records().tobytes()
    empty = frames[0][:0]
    got2, pko2 = rows.call([empty, empty, frames[2][5:]])
    want2, want_pko2 = model.call([empty, empty, frames[2][5:]])
    assert pko2 == want_pko2 and pko2[:3] == [0, 0, 0]
    same_stream(np.concatenate([got1[2], got2[2]]), want_whole[2], "the clipped frame presented again")
    assert BM.canon(rows.records(), last_packets=False).tobytes() == BM.canon(whole.records(), last_packets=False).tobytes()


def test_a_decreasing_pair_is_an_empty_stream():
    """offsets [4, 0, 5, 9]: stream 0 (4 -> 0) is empty and its record untouched, streams 1 and 2 own frames 0..5 and 5..9 as ever"""
    frames = three_streams()
    rows, model = Rows(KBCH, 3, 16), BM.Rows(KBCH, 3)
    rows.set_record(0, PATTERN)
    got, pko = rows.call([frames[0][:0], frames[0], frames[1]], offsets=[4, 0, 5, 9])
    want, want_pko = model.call([frames[0][:0], frames[0], frames[1]])
    assert pko == want_pko and pko[:2] == [0, 0]
    for s in range(3):
        same_stream(got[s], want[s], f"stream {s}")
    rec = rows.records()
    assert rec[0].tobytes() == PATTERN.tobytes() and rec[1:].tobytes() == model.records()[1:].tobytes()


def test_a_memset_of_one_record_resets_that_stream():
    import torch
    rt = T.hip_runtime()
    rt.hipMemsetAsync.restype = C.c_int
    rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    frames = three_streams()
    rows, model = Rows(KBCH, 3, 16), BM.Rows(KBCH, 3)
    rows.call([f[:3] for f in frames])
    model.call([f[:3] for f in frames])
    assert rt.hipMemsetAsync(rows.state_ptr(1), 0, 256, T.stream()) == 0
    model.reset(1)
    got, pko = rows.call([f[3:] for f in frames])
    want, want_pko = model.call([f[3:] for f in frames])
    torch.cuda.synchronize()
    assert pko == want_pko
    for s in range(3):
        same_stream(got[s], want[s], f"stream {s}")
    assert BM.canon(rows.records()).tobytes() == BM.canon(model.records()).tobytes()
    fresh = T.OracleBbDeheader(KBCH)
    same_stream(got[1], fresh.work(frames[1][3:]), "the reset stream is a block as constructed")
    assert model.counters()[0]["bbframes"] == 5 and model.counters()[1]["bbframes"] == 1


# ------------------------------------------------------------------ 5. end to end
PLSC, GOLD = L.PLSC, L.GOLD
FRAME_LEN = L.M.pls_parse(PLSC)["plframe_len"]
SLOT = FRAME_LEN + 90
MAX_SLOTS = 18


def shaped_carrier(bbframes, lead, seed):
    """loopback.shaped_six_frames with the encoder's input given: six BBFRAMEs through the scrambling encoder, the PL framer over
    loopback.SEQ6 behind `lead` random QPSK symbols, the pulse shaper. Returns (samples on the device float32 [ns, 2], ns)."""
    import torch
    st = T.stream()
    rng = np.random.default_rng(seed)
    enc = FecEncoder(max_frames=6, **L.QPSK_1_4_SHORT)
    enc.set_scramble(True)
    assert bbframes.shape == (6, enc.in_bytes)
    lay = plframer_layout(L.SEQ6)
    d_xfec = torch.zeros((6, enc.n_syms, 2), dtype=torch.float32, device="cuda")
    enc.work_device(torch.from_numpy(np.ascontiguousarray(bbframes)).cuda().data_ptr(), 6, d_syms=d_xfec.data_ptr(), stream=st)
    fr = PlFramer(GOLD, max_frames=len(L.SEQ6))
    fr.set_sequence(L.SEQ6)
    history = pulse_geometry(L.SPS, L.RRC_DELAY)[1]
    n_all = lead + lay["out_syms"] + 90 + history + 64
    d_x = torch.zeros((n_all, 2), dtype=torch.float32, device="cuda")
    d_x[:lead] = torch.from_numpy(L.P.qpsk(rng, lead).astype(np.complex64).view(np.float32).reshape(-1, 2)).cuda()
    fr.work_device(d_xfec.data_ptr(), len(L.SEQ6), L.SEQ6[-1], d_x.data_ptr() + 8 * lead, st)
    ps = PulseShaper(L.SPS, taps=L.unit_amplitude_taps(L.SPS, L.ROLLOFF, L.RRC_DELAY, L.TAU), max_symbols=n_all)
    d_y = torch.zeros((n_all * L.SPS, 2), dtype=torch.float32, device="cuda")
    ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), n_all * L.SPS, st)
    torch.cuda.synchronize()
    for o in (ps, fr, enc):
        o.close()
    return d_y, n_all * L.SPS


def test_samples_to_ts_packets_without_a_host_read_of_the_offsets():
    """Three carriers (tests/test_plsync_batch_gpu.py's end-to-end streams), each six BBFRAMEs that a BbFramer made from its own TS
    packets: batched SymbolSync -> PlSyncBatch -> gather -> PlCoarseBatch -> ONE strided front-end launch -> ONE FecChain call -> ONE
    bbdeheader_rows_device call with the gather's d_offsets, which the host reads only afterwards. The tracker locks on the first data
    frame, so each carrier's frames 1..5 arrive: its range of d_ts_out holds its own packets and nothing else, from behind the
    resynchronisation skip the oracle predicts for frame 1."""
    import torch
    st = T.stream()
    kbch = capi_kbch()
    ups, bbs, tx = [], [], []
    for c, (lead, seed) in enumerate(((400, 5101), (733, 5102), (150, 5103))):
        framer = BbFramer(framesize=capi.FECFRAME_SHORT, rate="C1_4", max_frames=6)
        assert framer.kbch_bytes * 8 == kbch
        u = T.ts_up_stream(framer.need(6) + 1, np.random.default_rng(7000 + c))
        bbs.append(framer.work(u, 6))
        framer.close()
        ups.append(u)
        tx.append(shaped_carrier(bbs[-1], lead, seed))
    ns = max(n for _, n in tx)
    d_y = torch.zeros((3, ns, 2), dtype=torch.float32, device="cuda")
    for i, (y, n) in enumerate(tx):
        d_y[i, :n] = y
    ss = SymbolSync(sps=L.SPS, loop_bw=0.01, damping=1.0, rolloff=L.ROLLOFF, interp_method=0, max_streams=3, max_samples=ns)
    d_sym = torch.zeros((3, ns, 2), dtype=torch.float32, device="cuda")
    ss.work_device(d_y.data_ptr(), ns, [n for _, n in tx], d_sym.data_ptr(), ns, ns, 0, 0, st)
    n_out, _, status = ss.finish()  # (the symbol counts are host arrays of the search: the one host read, in front of it)
    assert status.tolist() == [0, 0, 0]
    ps = PlSyncBatch(plsc=-1, max_streams=3, max_symbols=max(ns, PlSync.MIN_SYMBOLS), max_frames=16)
    pcb = PlCoarseBatch(1, PLSC, max_streams=3, max_slots=MAX_SLOTS)
    fe = PlFrontEnd(GOLD, PLSC, max_frames=MAX_SLOTS)
    chain = FecChain(group_size=4, max_frames=MAX_SLOTS, max_trials=25, **L.QPSK_1_4_SHORT)
    chain.set_descramble(True)
    assert chain.msg_bytes * 8 == kbch
    z = lambda n, dtype=torch.float32: torch.zeros(n, dtype=dtype, device="cuda")  # noqa: E731
    d_f, d_slots, d_off = z(3 * 16 * 16, torch.uint8), z(MAX_SLOTS * SLOT * 2), z(4, torch.int32)
    d_fo, d_cc, d_rx = z(MAX_SLOTS), z(MAX_SLOTS, torch.int32), z(MAX_SLOTS * fe.xfecframe_len * 2)
    d_n0, d_msg = torch.full((1,), 0.02, dtype=torch.float32, device="cuda"), z(MAX_SLOTS * chain.msg_bytes, torch.uint8)
    rows = Rows(kbch, 3, MAX_SLOTS)
    rows.out.fill_(FILL)
    ps.work_device(d_sym.data_ptr(), ns, [0, 0, 0], n_out, d_f.data_ptr(), st)
    ps.gather_device(d_sym.data_ptr(), ns, d_f.data_ptr(), 3, PLSC, d_slots.data_ptr(), MAX_SLOTS, d_off.data_ptr(), 0, st)
    pcb.work_device(d_slots.data_ptr(), SLOT, d_off.data_ptr(), 3, 0, d_fo.data_ptr(), d_cc.data_ptr(), 0, st)
    # (the frame counts of these two launches are host arguments: all slots, so that no count is read back)
    fe.work_strided_device(d_slots.data_ptr(), SLOT, MAX_SLOTS, d_cc.data_ptr(), d_fo.data_ptr(), d_rx.data_ptr(), st)
    chain.enqueue_device(d_rx.data_ptr(), MAX_SLOTS, d_n0.data_ptr(), 1, d_msg.data_ptr(), 0, 0, st)
    bbdeheader_rows_device(d_msg.data_ptr(), kbch, d_off.data_ptr(), 3, MAX_SLOTS, rows.state_ptr(), rows.work.data_ptr(), rows.g["work_bytes"],
                           rows.out.data_ptr(), rows.g["out_bytes"], rows.pko.data_ptr(), 0, st)
    chain.finish()
    ps.finish()
    torch.cuda.synchronize()
    assert d_off.cpu().tolist() == [0, 5, 10, 15]
    pko, out = rows.pko.cpu().numpy()[:4], rows.out.cpu().numpy()
    assert (out[int(pko[3]) * 188:] == FILL).all()
    model = BM.Rows(kbch, 3)
    want, want_pko = model.call([bb[1:6] for bb in bbs])
    assert pko.tolist() == want_pko
    dflb = (kbch - 80) // 8
    for c in range(3):
        got = out[int(pko[c]) * 188:int(pko[c + 1]) * 188]
        same_stream(got, want[c], f"carrier {c} against the oracle")
        # its own packets: from the first that starts in frame 1 (ceil(374 / 188) packets start in frame 0: the skip ends where packet
        # `first` starts) to the last whose CRC byte lies in frame 5
        first = -(-dflb // 188)
        n = got.size // 188
        assert n == (6 * dflb) // 188 - first and n >= 8
        same_stream(got, ups[c][first * 188:(first + n) * 188], f"carrier {c}: its own TS packets")
    assert BM.canon(rows.records()).tobytes() == BM.canon(model.records()).tobytes()
    assert [c["errors"] for c in model.counters()] == [0, 0, 0] and [c["synched"] for c in model.counters()] == [1, 1, 1]
    for o in (chain, fe, pcb, ps, ss):
        o.close()


def capi_kbch():
    from dvbs2rx_amd import get_fec_info
    return int(get_fec_info(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4")["bch_k"])
