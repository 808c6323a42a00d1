"""What the tests of the batched PL stages share (tests/test_plsync_batch_gpu.py, tests/test_plsync_batch_stream_gpu.py): the five
streams of one batch on the device, built once and never written again, the loop that follows every stream's own `consumed` through a
PlSyncBatch, the same loop over a single-stream PlSync -- the oracle: per stream every record, count, `consumed` and state of the batch
must be its bytes --, and the gather of a batch. All short QPSK 1/4 frames with pilots (PLFRAME 8370 symbols), loopback.SEQ6."""
import functools
from types import SimpleNamespace as NS

import numpy as np

import fec_testlib as T
import loopback as L
import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import Awgn, PlSync, PlSyncBatch, awgn_sigma, capi

PLSC, GOLD = L.PLSC, L.GOLD
FRAME_LEN = M.pls_parse(PLSC)["plframe_len"]
SLOT = FRAME_LEN + 90
MAX_FRAMES = 16
SIZES = (33461, 35003, 39999, 34567)  # the call sizes of tests/test_plsync_gpu.py: a pending frame always fits into the next call
MAX_SYMBOLS = 1 << 16                 # above every stream here and every call size

# the batch: three SEQ6 streams with different seeds and leads, the second behind noise at 10 dB; noise alone; nothing
CLEAN_A, NOISY, NOISE_ONLY, EMPTY, CLEAN_B = range(5)
SEQ = {CLEAN_A: (1400, 4101), NOISY: (701, 4102), CLEAN_B: (2333, 4103)}  # stream -> (lead, seed)
ES_N0_DB = 10.0
NOISE_LEN = 41003


def zeros(n, dtype="float32"):
    import torch
    return torch.zeros(int(n), dtype=getattr(torch, dtype), device="cuda")


def records(t, n_streams, max_frames=MAX_FRAMES):
    return t.cpu().numpy().view(PlSync.FRAME_DTYPE).reshape(n_streams, max_frames)


@functools.lru_cache(None)
def streams():
    """NS(d_x: float32 [5, stride, 2] on the device, x: the same on the host as complex64 [5, stride] (read-only), n: the five lengths,
    stride, sent: stream -> the encoder's input bytes [6, in_bytes])"""
    import torch
    tx = {s: L.transmit_symbols(L.SEQ6, 6, GOLD, lead, seed, flush=0) for s, (lead, seed) in SEQ.items()}
    n = [0] * 5
    for s, t in tx.items():
        n[s] = t[2]
    n[NOISE_ONLY] = NOISE_LEN
    stride = (max(n) + 7) | 1  # odd: odd rows of the batch start at odd symbol indices: 8-byte aligned and no more
    assert max(n) <= MAX_SYMBOLS and stride % 2 == 1
    d_x = torch.zeros((5, stride, 2), dtype=torch.float32, device="cuda")
    for s, t in tx.items():
        d_x[s, :n[s]] = t[1][:n[s]]
    ch = Awgn(seed=77, sigma=awgn_sigma(ES_N0_DB), max_streams=1, max_samples=stride)
    row = d_x.data_ptr() + 8 * stride * NOISY
    ch.work_device(row, stride, n[NOISY], 1, row, stride, first_stream=NOISY, first_index=0, stream=T.stream())
    torch.cuda.synchronize()
    ch.close()
    rng = np.random.default_rng(4104)
    noise = ((rng.normal(size=NOISE_LEN) + 1j * rng.normal(size=NOISE_LEN)) * np.sqrt(0.5)).astype(np.complex64)
    d_x[NOISE_ONLY, :NOISE_LEN] = torch.from_numpy(noise.view(np.float32).reshape(-1, 2)).cuda()
    torch.cuda.synchronize()
    x = d_x.cpu().numpy().reshape(5, stride * 2).view(np.complex64)
    x.setflags(write=False)
    return NS(d_x=d_x, x=x, n=n, stride=stride, sent={s: t[0] for s, t in tx.items()})


def sizes_of(s):
    """the call sizes of stream s: the cycle of SIZES, begun at another point for every stream"""
    k = (0, 1, 3, 3, 2)[s]  # the three SEQ6 streams (0, 1, 4) each begin at another size
    return SIZES[k:] + SIZES[:k]


def run_batch(ps, d_x, stride, lengths, sizes=None, d_f=None, first0=None, start_call=None):
    """Every stream through ps from its first symbol to its last, each following its OWN `consumed` through first[]. sizes: None (one
    call holds a whole stream) or stream -> the cycle of its call sizes. A stream that has been presented to its end takes part in the
    later calls with n_syms = 0. start_call: None, or per stream the call with which it begins: in front of it the stream takes part
    with n_syms = 0, and its cycle of sizes begins with its own first call. Returns NS(calls: per stream the list of (n_syms, records
    bytes, n_frames, consumed, state) of the calls it took part in, recs: per stream all its records, pos, state, n_calls, d_f: the record buffer of the LAST call)."""
    S = len(lengths)
    d_f = zeros(S * ps.max_frames * 16, "uint8") if d_f is None else d_f
    first0 = [0] * S if first0 is None else first0
    start_call = [0] * S if start_call is None else start_call
    pos, done, calls, state = [0] * S, [n == 0 for n in lengths], [[] for _ in range(S)], [None] * S
    i = 0
    while not all(done):
        idle = [done[s] or i < start_call[s] for s in range(S)]
        n = [0 if idle[s] else min(lengths[s] - pos[s], sizes[s][(i - start_call[s]) % len(sizes[s])] if sizes else lengths[s]) for s in range(S)]
        ps.work_device(d_x.data_ptr(), stride, [first0[s] + pos[s] for s in range(S)], n, d_f.data_ptr(), T.stream())
        nf, consumed, st = ps.finish()
        recs = records(d_f, S, ps.max_frames)
        for s in range(S):
            if idle[s]:
                assert (nf[s], consumed[s]) == (0, 0), f"stream {s} was presented nothing and reports {nf[s]} frames, {consumed[s]} consumed"
                assert state[s] is None or st[s] == state[s]
                continue
            assert 0 <= consumed[s] <= n[s] and 0 <= nf[s] <= ps.max_frames
            calls[s].append((n[s], recs[s, :nf[s]].tobytes(), int(nf[s]), int(consumed[s]), int(st[s])))
            at_end = pos[s] + n[s] == lengths[s]
            pos[s] += int(consumed[s])
            state[s] = int(st[s])
            done[s] = at_end
            assert at_end or consumed[s] > 0
        i += 1
        assert i < 100
    allrecs = [np.frombuffer(b"".join(c[1] for c in calls[s]), PlSync.FRAME_DTYPE) for s in range(S)]
    return NS(calls=calls, recs=allrecs, pos=pos, state=state, n_calls=i, d_f=d_f)


def run_single(d_row, length, sizes=None, max_frames=MAX_FRAMES, max_symbols=MAX_SYMBOLS):
    """the same loop over a fresh single-stream PlSync: d_row is the address of the stream's first symbol. Returns the stream's list of
    calls as run_batch gives it, and the handle (open: after its last search)."""
    ps = PlSync(plsc=-1, max_symbols=max_symbols, max_frames=max_frames)
    d_f = zeros(max_frames * 16, "uint8")
    pos, calls, i = 0, [], 0
    while length:
        n = min(length - pos, sizes[i % len(sizes)] if sizes else length)
        ps.work_device(d_row + 8 * pos, n, d_f.data_ptr(), T.stream())
        nf, consumed, st = ps.finish()
        calls.append((n, records(d_f, 1, max_frames)[0, :nf].tobytes(), nf, consumed, st))
        at_end = pos + n == length
        pos += consumed
        i += 1
        if at_end:
            break
        assert consumed > 0 and i < 100
    return calls, ps, d_f


@functools.lru_cache(None)
def single_reference(s, cut):
    """the calls of stream s of streams() through a single-stream handle: whole (cut False) or in its own call sizes"""
    c = streams()
    calls, ps, _ = run_single(c.d_x.data_ptr() + 8 * c.stride * s, c.n[s], sizes_of(s) if cut else None)
    ps.close()
    return calls


@functools.lru_cache(None)
def model_records(s):
    """plsync_model's tracker over clean stream s: (records, consumed, state, the metric's bound per index); the stream must be one
    the model vouches for (no decision within float32 rounding of a threshold or a tie)"""
    x = streams().x[s, :streams().n[s]]
    met, bound = P.metric(x)
    log = []
    recs, consumed, state, visits = P.track(met, P.make_decoder(x, log=log), 3, -1, 64)
    assert P.guard(dict(met=met, bound=bound, visits=visits, log=log)) == (0, 0)
    return recs, consumed, state, bound


def gather(ps, d_x, stride, d_f, n_streams, wanted=PLSC, max_slots=None, room=None):
    """gather_device of the last search of ps. room: slots the buffer has (max_slots when None); behind it lie 64 sentinel words. Returns
    NS(slots: complex64 [room, SLOT] on the host, d_slots, offsets, d_off, slot_record [room, 2], tail: the words behind the buffer)"""
    import torch
    max_slots = n_streams * ps.max_frames if max_slots is None else max_slots
    room = max_slots if room is None else room
    d_slots = T.sentinel(room * SLOT * 2 + T.PAD)
    d_off = torch.full((n_streams + 1,), -7, dtype=torch.int32, device="cuda")
    d_rec = torch.full((max(room, 1) * 2,), -7, dtype=torch.int32, device="cuda")
    ps.gather_device(d_x.data_ptr(), stride, d_f.data_ptr(), n_streams, wanted, d_slots.data_ptr(), max_slots, d_off.data_ptr(), d_rec.data_ptr(), T.stream())
    torch.cuda.synchronize()
    words = d_slots.cpu().numpy()
    return NS(slots=words[:room * SLOT * 2].view(np.complex64).reshape(room, SLOT), d_slots=d_slots, offsets=d_off.cpu().numpy(), d_off=d_off,
              slot_record=d_rec.cpu().numpy()[:room * 2].reshape(room, 2), d_slot_record=d_rec, tail=words[room * SLOT * 2:].view(np.uint32))


def selected(recs, length, pos0=0, wanted=PLSC):
    """indices of the records gather takes: locked, of the wanted PLSC (every reported record lies whole inside its buffer)"""
    return [i for i, r in enumerate(recs) if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == wanted]


def make_batch(n_streams, max_frames=MAX_FRAMES, max_symbols=MAX_SYMBOLS, plsc=-1):
    return PlSyncBatch(plsc=plsc, max_streams=n_streams, max_symbols=max_symbols, max_frames=max_frames)
