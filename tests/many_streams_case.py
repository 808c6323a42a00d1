"""What tests/test_many_streams_gpu.py (the device) and tests/test_many_streams_case.py (the conditions on the inputs, from the models
alone) share: the batched stages at 17, 256, 257 and 1024 streams. A batch of S streams is built from a small set of VARIANTS -- a variant
is a stream whose reference is computed once and cached --, assigned to the streams by a seeded generator, so that the assignment is
periodic in nothing: a kernel that reads stream s - 16, s mod 256 or a 32-bit product of s reads another variant. The streams at the
indices where a kernel changes its path (EDGES and S - 1) are forced to variants that produce output.
  1. PlSyncBatch / PlCoarseBatch: 13 variants of the rows of plsync_batch_case.streams(), the oracle a single PlSync / PlCoarse;
  2. the rotator rows and the control step: random records, the oracle S launches of one row and rotator_rows_model;
  3. the de-header rows: per-stream frames of bbdeheader_rows_model's generators, the oracle bbdeheader_rows_model.Rows."""
import functools
from types import SimpleNamespace as NS

import numpy as np

import bbdeheader_rows_model as BM
import fec_testlib as T
import plsync_batch_case as B
import rotator_rows_model as RM
from dvbs2rx_amd import ROTATOR_STATE, PlCoarse, PlSync

EDGES = (0, 15, 16, 17, 255, 256, 257)  # around the 16 wavefronts of the count kernel and the 256 lanes of the prefix and control kernels
LAGS = (1, 16, 64, 256)
LAG_SHARE = 0.75


def edges(S):
    return sorted({e for e in EDGES + (S - 1,) if e < S})


def assign(S, n_variants, productive, seed):
    """variant[s] for S streams: uniform over n_variants, the edge streams redrawn among `productive` where they are not"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, n_variants, S)
    for e in edges(S):
        if int(v[e]) not in productive:
            v[e] = productive[int(rng.integers(0, len(productive)))]
    v.setflags(write=False)
    return v


def lag_shares(v):
    """lag -> the share of the streams s >= lag whose variant differs from that of stream s - lag"""
    v = np.asarray(v)
    return {d: float(np.mean(v[d:] != v[:-d])) for d in LAGS if d < len(v)}


# ------------------------------------------------------------------ 1. search, gather and coarse estimate
PL_S = (17, 257, 1024)
PL_CAPPED_FROM = 1024  # from here on every stream is capped at PlSync.MIN_SYMBOLS symbols: 137 MB of metric and 273 MB of symbols
TRIMS = (0, 1, 350)    # symbols cut off the front: below the smallest lead (701), so content and every sof_index differ per trim
PL_BASES = (B.CLEAN_A, B.NOISY, B.NOISE_ONLY, B.CLEAN_B)
PL_VARIANTS = tuple((b, t) for b in PL_BASES for t in TRIMS) + ((B.EMPTY, 0),)  # (row of streams(), trim): 13
PL_PRODUCTIVE = tuple(v for v, (b, _) in enumerate(PL_VARIANTS) if b in (B.CLEAN_A, B.CLEAN_B))  # locked, with selected records
PL_SEED = {17: 1702, 257: 25701, 1024: 102401}
assert min(lead for lead, _ in B.SEQ.values()) > max(TRIMS) and len(PL_VARIANTS) == 13


def pl_assignment(S):
    return assign(S, len(PL_VARIANTS), PL_PRODUCTIVE, PL_SEED[S])


def pl_start_calls(S):
    """the call with which stream s begins in the cut runs: streams of one variant do not move in lockstep"""
    return np.random.default_rng(PL_SEED[S] + 1).integers(0, 3, S).tolist()


def pl_capped(S):
    return S >= PL_CAPPED_FROM


@functools.lru_cache(None)
def pl_rows(capped):
    """the 13 variants as rows: NS(d: float32 [13, stride, 2] on the device, x: the same on the host as complex64 (read-only), n, stride)"""
    import torch
    c = B.streams()
    cap = PlSync.MIN_SYMBOLS if capped else B.MAX_SYMBOLS
    n = [min(c.n[b] - t, cap) if b != B.EMPTY else 0 for b, t in PL_VARIANTS]
    stride = (PlSync.MIN_SYMBOLS | 1) if capped else c.stride  # odd, as streams()'s
    assert stride % 2 == 1 and max(n) <= stride
    d = torch.zeros((len(PL_VARIANTS), stride, 2), dtype=torch.float32, device="cuda")
    for v, (b, t) in enumerate(PL_VARIANTS):
        d[v, :n[v]] = c.d_x[b, t:t + n[v]]
    torch.cuda.synchronize()
    x = d.cpu().numpy().reshape(len(PL_VARIANTS), stride * 2).view(np.complex64)
    x.setflags(write=False)
    return NS(d=d, x=x, n=n, stride=stride)


@functools.lru_cache(None)
def pl_batch(S):
    """NS(d_x: float32 [S, stride, 2], written once by index_select of the variants' rows, stride, variant, lengths)"""
    import torch
    rows, variant = pl_rows(pl_capped(S)), pl_assignment(S)
    d_x = rows.d.index_select(0, torch.from_numpy(np.array(variant)).cuda())
    torch.cuda.synchronize()
    return NS(d_x=d_x, stride=rows.stride, variant=variant, lengths=[rows.n[v] for v in variant])


@functools.lru_cache(None)
def pl_reference(v, mode):
    """the calls of variant v through a single-stream PlSync, as plsync_batch_case.run_single gives them. mode: "whole" (one call),
    "cut" (its base's cycle of call sizes) or "capped" (the capped variant in one call, max_symbols = MIN_SYMBOLS as the batch's)"""
    rows = pl_rows(mode == "capped")
    calls, ps, _ = B.run_single(rows.d.data_ptr() + 8 * rows.stride * v, rows.n[v], B.sizes_of(PL_VARIANTS[v][0]) if mode == "cut" else None,
                                max_symbols=PlSync.MIN_SYMBOLS if mode == "capped" else B.MAX_SYMBOLS)
    ps.close()
    return calls


def pl_records(calls):
    return np.frombuffer(b"".join(c[1] for c in calls), PlSync.FRAME_DTYPE)


@functools.lru_cache(None)
def pl_selected(v, mode):
    """(the record indices gather takes of variant v's whole-stream reference, their slots complex64 [k, SLOT] cut from the variant's
    row on the host)"""
    rows = pl_rows(mode == "capped")
    recs = pl_records(pl_reference(v, mode))
    sel = B.selected(recs, rows.n[v])
    slots = np.zeros((len(sel), B.SLOT), np.complex64)
    for k, f in enumerate(sel):
        sof = int(recs[f]["sof_index"])
        assert 0 <= sof and sof + B.SLOT <= rows.n[v]
        slots[k] = rows.x[v, sof:sof + B.SLOT]
    slots.setflags(write=False)
    return sel, slots


@functools.lru_cache(None)
def pl_coarse_reference(v, mode):
    """two calls of a single PlCoarse(1, -1) over variant v's selected frames: [(foffset, corrected, new_est)] * 2"""
    import torch
    _, slots = pl_selected(v, mode)
    k = len(slots)
    if k == 0:
        return [(np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))] * 2
    d_slots = torch.from_numpy(np.array(slots).view(np.float32)).cuda()
    d_plsc = torch.full((k,), B.PLSC, dtype=torch.uint8, device="cuda")
    pc = PlCoarse(1, -1, max_frames=k)
    out = []
    for _ in range(2):
        o = [B.zeros(k), B.zeros(k, "int32"), B.zeros(k, "int32")]
        pc.work_device(d_slots.data_ptr(), B.SLOT, k, d_plsc.data_ptr(), *[t.data_ptr() for t in o], stream=T.stream())
        torch.cuda.synchronize()
        out.append(tuple(t.cpu().numpy() for t in o))
    pc.close()
    return out


@functools.lru_cache(None)
def pl_searched(S):
    """(handle, the run) behind ONE search of every whole stream of pl_batch(S); the handle stays open for the gathers of the module"""
    b = pl_batch(S)
    ps = B.make_batch(S, max_symbols=PlSync.MIN_SYMBOLS if pl_capped(S) else B.MAX_SYMBOLS)
    return ps, B.run_batch(ps, b.d_x, b.stride, b.lengths)


# ------------------------------------------------------------------ 2. rotator rows and the control step
ROT_S = (257, 1024)
ROT_N = (1, 257, 513)
ROT_BASE = (1 << 31) + 1
ROT_SEED = {257: 25702, 1024: 102402}
CONTROL_S = (256, 257, 1024)
CONTROL_KINDS = ("coarse", "fine", "coarse-fine", "fine-coarse", "nothing", "nan", "half")  # scenario() of tests/test_rotator_rows_gpu.py
CONTROL_SEED = {256: 25612, 257: 25716, 1024: 102403}
CONTROL_AT, COARSE_SCALE, FINE_SCALE = 1 << 33, 1.0, 0.5  # (coarse scale 1: the estimate 0.5 of "half" does not apply)
CONTROL_CUT = 5


def _u64(rng):
    return int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))


def random_records(S, seed):
    """S records as dicts of Python ints: random 64-bit phase, inc, index (signed) and reserved"""
    rng = np.random.default_rng(seed)
    return [RM.state(_u64(rng), _u64(rng), _u64(rng) - (1 << 63), _u64(rng)) for _ in range(S)]


@functools.lru_cache(None)
def rot_records(S):
    """random records; inc 0, 2^63 and 2^64 - 1 on streams 0, 256 and S - 1 (2^63 on stream 255 where 256 is the last)"""
    states = random_records(S, ROT_SEED[S])
    for s, inc in ((0, 0), (256 if S - 1 != 256 else 255, 1 << 63), (S - 1, (1 << 64) - 1)):
        states[s]["inc"] = inc
    return states


@functools.lru_cache(None)
def rot_input(S, n):
    """complex64 [S, n] (read-only): the rows of test_rotator_rows_gpu.samples() cycled, begun at a point of the stream's own and scaled
    per stream, so that no two rows hold equal samples"""
    import test_rotator_rows_gpu as R
    base = R.samples()
    x = np.stack([base[s % len(R.INCS), 7 * s:7 * s + n] for s in range(S)]) * (1.0 + np.arange(S, dtype=np.float32) / 64.0)[:, None]
    x = np.ascontiguousarray(x, np.complex64)
    assert len({r.tobytes() for r in x}) == S
    x.setflags(write=False)
    return x


def rot_model_streams(S):
    """the eight streams compared with the float64 evaluation: the edges and two inside"""
    pick = []
    for s in (0, 255, 256, S - 1, 257, 17, S // 2, S // 3, 16, 15):
        if s < S and s not in pick and len(pick) < 8:
            pick.append(s)
    return sorted(pick)


@functools.lru_cache(None)
def control_case(S):
    """NS(variant: kind * 5 + slots per stream, offsets, total, arrays: (coarse_foffset, coarse_corrected, new_est, fine_foffset,
    fine_valid) over the slots, before: the records). The edge streams have a steering kind and at least one slot."""
    import test_rotator_rows_gpu as R
    productive = tuple(k * 5 + n for k in range(4) for n in range(1, 5))
    variant = assign(S, len(CONTROL_KINDS) * 5, productive, CONTROL_SEED[S])
    counts = [int(v) % 5 for v in variant]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(offsets[-1])
    arrays = [np.zeros(total, t) for t in (np.float32, np.int32, np.int32, np.float32, np.int32)]
    for s, v in enumerate(variant):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if a == b:
            continue
        for dst, src in zip(arrays, R.scenario(CONTROL_KINDS[int(v) // 5], b - a)):
            dst[a:b] = src
    return NS(variant=variant, offsets=offsets.tolist(), total=total, arrays=arrays, before=random_records(S, CONTROL_SEED[S] + 1))


def control_model(S, max_slots, fine):
    """(applied, delta, the records afterwards) of rotator_rows_model.control"""
    c = control_case(S)
    cf, cc, ne, ff, fv = c.arrays
    states = [dict(st) for st in c.before]
    applied, delta = RM.control(c.offsets, max_slots, cf, cc, ne, ff if fine else None, fv if fine else None, COARSE_SCALE, FINE_SCALE, CONTROL_AT,
                                states)
    return applied, delta, RM.to_records(states, ROTATOR_STATE)


# ------------------------------------------------------------------ 3. de-header rows
DH_S = (256, 257, 1024)
KBCH = 3072
DH_KINDS = ("healthy", "fuzzed", "bad")
DH_KIND_SHARE = (0.47, 0.47, 0.06)
DH_MAX = 6                                  # frames per stream: 0..6
DH_LONG = {256: 131, 257: 256, 1024: 700}   # the stream of DH_LONG_FRAMES frames: more than one frame per scan thread (above 256 where S allows)
DH_LONG_FRAMES, DH_LONG_SEED = 300, 41      # (the fuzz seed of tests/test_bbdeheader_rows_gpu.py: it meets everything)
DH_SEED = {256: 25603, 257: 25703, 1024: 102404}
DH_SINGLES = 16


@functools.lru_cache(None)
def dh_frames(kind, seed):
    """DH_MAX frames of one stream (a shorter stream is their prefix), read-only"""
    if kind == "healthy":
        fr = BM.healthy(KBCH, DH_MAX, seed)[1]
    elif kind == "fuzzed":
        fr = BM.fuzzed(KBCH, 2 * DH_MAX, seed)[:DH_MAX]  # (the generator loses frames on the way)
    else:
        fr = BM.bad_headers(KBCH, DH_MAX, seed)
    assert len(fr) == DH_MAX
    fr.setflags(write=False)
    return fr


@functools.lru_cache(None)
def dh_long():
    fr = BM.fuzzed(KBCH, DH_LONG_FRAMES + 20, DH_LONG_SEED)[:DH_LONG_FRAMES]
    assert len(fr) == DH_LONG_FRAMES
    fr.setflags(write=False)
    return fr


@functools.lru_cache(None)
def dh_case(S):
    """NS(variant: kind * 7 + frames per stream, frames: per stream its BBFRAMEs, cut: per stream the frames of the first call, pieces: the
    two calls, each a list of S frame arrays, long). A variant here names the generator and the count; the frames are drawn with the
    stream's own seed, so no two streams carry the same bytes. The edge streams are healthy with at least two frames."""
    productive = tuple(n for n in range(2, DH_MAX + 1))  # kind 0
    rng = np.random.default_rng(DH_SEED[S])
    kinds = rng.choice(len(DH_KINDS), S, p=DH_KIND_SHARE)
    counts = rng.integers(0, DH_MAX + 1, S)
    variant = kinds * (DH_MAX + 1) + counts
    for e in edges(S):
        if int(variant[e]) not in productive:
            variant[e] = productive[int(rng.integers(0, len(productive)))]
    frames, cut = [], []
    for s, v in enumerate(variant):
        n = int(v) % (DH_MAX + 1)
        frames.append(dh_frames(DH_KINDS[int(v) // (DH_MAX + 1)], 9000 + s)[:n])
        # one stream in ten gets nothing in the first call, one in five everything; the others are cut inside
        r = rng.random()
        cut.append(0 if r < 0.1 else n if r < 0.3 or n < 2 else int(rng.integers(1, n)))
    for e in edges(S):
        cut[e] = max(cut[e], 1)  # an edge stream has packets in the first call
    long = DH_LONG[S]
    frames[long], cut[long] = dh_long(), 143
    variant[long] = len(DH_KINDS) * (DH_MAX + 1)  # a variant of its own (at S = 257 it is the edge stream 256: it has packets in both calls)
    variant.setflags(write=False)
    pieces = [[f[:c] for f, c in zip(frames, cut)], [f[c:] for f, c in zip(frames, cut)]]
    return NS(variant=variant, frames=frames, cut=cut, pieces=pieces, long=long)


@functools.lru_cache(None)
def dh_model(S):
    """the oracle over the two calls: per call NS(out: the TS bytes per stream, pko, records, counters)"""
    c = dh_case(S)
    m = BM.Rows(KBCH, S)
    calls = []
    for piece in c.pieces:
        out, pko = m.call(piece)
        calls.append(NS(out=out, pko=pko, records=m.records(), counters=m.counters()))
    return calls


def dh_single_streams(S):
    """the streams also compared with a single BbDeheader handle: the edges, the long stream, and others up to DH_SINGLES"""
    pick = sorted(set(edges(S)) | {dh_case(S).long})
    rng = np.random.default_rng(DH_SEED[S] + 2)
    while len(pick) < DH_SINGLES:
        s = int(rng.integers(0, S))
        if s not in pick:
            pick.append(s)
    return sorted(pick)
