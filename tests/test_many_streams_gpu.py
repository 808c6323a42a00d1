"""GPU: the batched stages at 17, 256, 257 and 1024 streams (tests/many_streams_case.py holds the inputs, the assignments and the cached
references; tests/test_many_streams_case.py asserts the conditions on them). The five- and six-stream tests of these stages leave most of
their batch code unrun: the second trip of a wavefront of plsync_batch_count_kernel (S = 17) and its whole LDS array (1024), the scan
across wavefronts and the chunks of bbdh_rows_prefix_kernel (256: one stream per thread; 257: two, the upper threads empty; 1024: four),
the second workgroup of rotator_control_kernel and the guard of a partly filled one (256, 257, 1024), and every per-stream stride of the
kernels that take the stream from blockIdx at a stream index above five.
The oracle is the one of the small tests: the single-stream handle of the stage (PlSync, PlCoarse, BbDeheader), a rotator_rows_device
call of one row (tied to Rotator by test_rotator_rows_gpu.test_rows_equal_single_handles), or the Python model (rotator_rows_model,
bbdeheader_rows_model.Rows). Everything is bit for bit or byte for byte, but the rotated rows against float64 (rotator_rows_model.rotate's
derived bound). Every test prints S, the variants met and the totals compared."""
import numpy as np
import pytest

import bbdeheader_rows_model as BM
import fec_testlib as T
import loopback as L
import many_streams_case as C
import plsync_batch_case as B
import rotator_rows_model as RM
import test_bbdeheader_rows_gpu as D
import test_rotator_rows_gpu as R
from dvbs2rx_amd import (ROTATOR_STATE, BbDeheader, PlCoarseBatch, bbdeheader_state_counters, capi, rotator_control_device, rotator_rows_device)

pytestmark = pytest.mark.gpu

SLOT = B.SLOT


def mode_of(S, cut=False):
    return "cut" if cut else "capped" if C.pl_capped(S) else "whole"


def same_calls(got, want, s, v):
    assert len(got) == len(want), f"stream {s} (variant {v}): {len(got)} calls against {len(want)} of the single handle"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"stream {s} (variant {v}), call {i}: n_syms, n_frames, consumed, state {g[0], g[2:]} against {w[0], w[2:]} of the single handle" + \
            ("" if g[1] == w[1] else "; the records differ")


# ------------------------------------------------------------------ 1. search, gather and coarse estimate
def test_pl_references():
    """from the single-stream references alone: every clean variant, trimmed or not, locks and reports loopback.SEQ6 from its whole
    stream, in one call or cut; capped at MIN_SYMBOLS it locks and has selected records, so an edge stream carries data; the trims give
    every variant of a base other record bytes"""
    for v in C.PL_PRODUCTIVE:
        for mode in ("whole", "cut", "capped"):
            calls = C.pl_reference(v, mode)
            recs = C.pl_records(calls)
            assert calls[-1][4] == capi.PLSYNC_LOCKED, (v, mode)
            if mode == "capped":
                assert [int(r["plsc"]) for r in recs] == L.SEQ6[:len(recs)] and len(recs) >= 2
            else:
                assert [int(r["plsc"]) for r in recs] == L.SEQ6
            if mode != "cut":
                assert len(C.pl_selected(v, mode)[0]) >= 1, (v, mode)
    for mode in ("whole", "capped"):
        assert len({C.pl_records(C.pl_reference(v, mode)).tobytes() for v in C.PL_PRODUCTIVE}) == len(C.PL_PRODUCTIVE)
    empty = len(C.PL_VARIANTS) - 1
    assert all(C.pl_reference(empty, mode) == [] for mode in ("whole", "cut", "capped"))
    print("PL references: selected records per variant, whole " + str([len(C.pl_selected(v, "whole")[0]) for v in range(13)])
          + ", capped " + str([len(C.pl_selected(v, "capped")[0]) for v in range(13)]))


@pytest.mark.parametrize("S", C.PL_S)
def test_search_whole_streams(S):
    """one call per stream: n_frames, consumed, state and the record bytes of every stream are its variant's single-stream reference
    (at 1024 of the variant capped at MIN_SYMBOLS symbols, in a handle with max_symbols = MIN_SYMBOLS)"""
    b = C.pl_batch(S)
    _, run = C.pl_searched(S)
    assert run.n_calls == 1
    for s, v in enumerate(b.variant):
        same_calls(run.calls[s], C.pl_reference(int(v), mode_of(S)), s, int(v))
    print(f"PL search, whole streams: S {S}, {len(set(b.variant.tolist()))} variants, {sum(len(r) for r in run.recs)} records compared")
    assert sum(len(r) for r in run.recs) > S


@pytest.mark.parametrize("S", (17, 257))
def test_search_cut_calls(S):
    """every stream follows its own `consumed` through its base's cycle of call sizes and begins with a call of its own (0..2): per
    stream the list of calls is its variant's cut reference; a stream presented nothing reports (0, 0) and keeps its state (run_batch)"""
    b = C.pl_batch(S)
    ps = B.make_batch(S)
    run = B.run_batch(ps, b.d_x, b.stride, b.lengths, [B.sizes_of(C.PL_VARIANTS[int(v)][0]) for v in b.variant], start_call=C.pl_start_calls(S))
    ps.close()
    for s, v in enumerate(b.variant):
        same_calls(run.calls[s], C.pl_reference(int(v), "cut"), s, int(v))
    print(f"PL search, cut calls: S {S}, {len(set(b.variant.tolist()))} variants, {run.n_calls} calls, {sum(len(k) for k in run.calls)} stream calls and "
          f"{sum(len(r) for r in run.recs)} records compared")
    assert run.n_calls >= 4 and sum(len(r) for r in run.recs) > S


def expected_gather(S):
    """(offsets [S + 1], slots complex64 [total, SLOT], slot_record [total, 2]) from the variants' references"""
    b, mode = C.pl_batch(S), mode_of(S)
    sel = [C.pl_selected(int(v), mode) for v in b.variant]
    offsets = np.concatenate([[0], np.cumsum([len(k[0]) for k in sel])])
    slots = np.concatenate([k[1] for k in sel])
    record = np.array([(s, f) for s, k in enumerate(sel) for f in k[0]], np.int32).reshape(-1, 2)
    return offsets, slots, record


@pytest.mark.parametrize("S", C.PL_S)
def test_gather(S):
    """behind the whole-stream search: d_offsets are the prefix sums of the references' selected counts, every slot is the SLOT symbols
    of its stream's row at the record's position, slot_record is (stream, record), nothing lies behind the last slot. At 257 once more
    with max_slots three below the total: the true total, and nothing behind slot max_slots - 1."""
    b = C.pl_batch(S)
    ps, run = C.pl_searched(S)
    offsets, slots, record = expected_gather(S)
    total = int(offsets[-1])
    for e in C.edges(S):
        assert offsets[e + 1] > offsets[e], f"edge stream {e} has no slot"
    for room in (total,) + ((total - 3,) if S == 257 else ()):
        g = B.gather(ps, b.d_x, b.stride, run.d_f, S, max_slots=room, room=room)
        assert g.offsets.tolist() == offsets.tolist(), f"d_offsets differ first at stream {np.flatnonzero(g.offsets != offsets)[0]}"
        assert (g.tail == T.SENTINEL).all(), "a write behind the last slot"
        bad = np.flatnonzero((g.slots.view(np.uint64) != slots[:room].view(np.uint64)).any(axis=1))
        assert bad.size == 0, f"{bad.size} of {room} slots differ, the first is slot {bad[0]} of stream {int(np.searchsorted(offsets, bad[0], 'right')) - 1}"
        assert np.array_equal(g.slot_record, record[:room])
    print(f"PL gather: S {S}, {len(set(b.variant.tolist()))} variants, {total} slots of {sum(len(r) for r in run.recs)} records compared")
    assert total > S // 2


@pytest.mark.parametrize("S", C.PL_S)
def test_coarse_estimate(S):
    """PlCoarseBatch(1, -1, max_streams=S, max_slots=total) over the gathered slots, two calls: foffset, corrected and new_est of every
    slot are a single PlCoarse's over the variant's selected frames in the same two calls; the second call continues every stream's
    window state"""
    import torch
    b, mode = C.pl_batch(S), mode_of(S)
    ps, run = C.pl_searched(S)
    offsets, _, _ = expected_gather(S)
    total = int(offsets[-1])
    g = B.gather(ps, b.d_x, b.stride, run.d_f, S, max_slots=total, room=total)
    assert g.offsets.tolist() == offsets.tolist()
    pcb = PlCoarseBatch(1, -1, max_streams=S, max_slots=total)
    d_plsc = torch.full((total,), B.PLSC, dtype=torch.uint8, device="cuda")
    seen = []
    for call in range(2):
        out = [B.zeros(total + 8), B.zeros(total + 8, "int32"), B.zeros(total + 8, "int32")]
        for o in out:
            o.fill_(-5)
        pcb.work_device(g.d_slots.data_ptr(), SLOT, g.d_off.data_ptr(), S, d_plsc.data_ptr(), *[o.data_ptr() for o in out], stream=T.stream())
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in out]
        for i, name in enumerate(("coarse_foffset", "coarse_corrected", "new_est")):
            want = np.concatenate([C.pl_coarse_reference(int(v), mode)[call][i] for v in b.variant])
            assert (got[i][total:] == -5).all(), f"call {call}: a write behind {name}"
            bad = np.flatnonzero(got[i][:total].view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (f"call {call}: {name} differs in {bad.size} of {total} slots, the first is slot {bad[0]} of stream "
                                   f"{int(np.searchsorted(offsets, bad[0], 'right')) - 1}: {got[i][bad[0]]} against {want[bad[0]]} of the single handle")
        seen.append(got)
    pcb.close()
    # (the comparison of the second call is not that of the first once more: a stream's first slot meets another window state)
    firsts = offsets[:-1][np.diff(offsets) > 0]
    moved = sum(1 for f in firsts if any(seen[0][i][f:f + 1].tobytes() != seen[1][i][f:f + 1].tobytes() for i in range(3)))
    print(f"PL coarse estimate: S {S}, {len(set(b.variant.tolist()))} variants, 2 x {total} slots compared; the first slot of {moved} of {firsts.size} "
          f"streams changes with the state the first call left")
    assert moved > 0


# ------------------------------------------------------------------ 2. rotator rows and the control step
@pytest.mark.parametrize("S", C.ROT_S)
@pytest.mark.parametrize("n", C.ROT_N)
def test_rotator_rows(S, n):
    """one launch over S rows at the strides n and n + 1 (the odd one alternates the 16-byte phase of the rows) with base_index
    2^31 + 1: every row equals the launch of that row and that record alone (n_streams = 1); eight rows, the edges among them, lie
    within the derived bound of the float64 evaluation; the records are not written, nor anything around or between the rows"""
    import torch
    x, states = C.rot_input(S, n), C.rot_records(S)
    recs = RM.to_records(states, ROTATOR_STATE)
    d_state = R.dev_state(recs)
    d_in = R.dev(x.view(np.float32))
    d_ref = T.sentinel(S * n * 2)
    for s in range(S):
        rotator_rows_device(d_in.data_ptr() + 8 * s * n, n, d_ref.data_ptr() + 8 * s * n, n, n, 1, C.ROT_BASE, d_state.data_ptr() + 32 * s, 0, T.stream())
    torch.cuda.synchronize()
    want = d_ref.cpu().numpy().view(np.uint32).reshape(S, n, 2)
    assert (want != T.SENTINEL).any(axis=(1, 2)).all()
    for stride in (n, n + 1):
        outs, _ = T.run_strided(lambda i, o: rotator_rows_device(i, stride, o, stride, n, S, C.ROT_BASE, d_state.data_ptr(), 0, T.stream()),
                                list(x), [n] * S, stride, stride)
        got = np.stack(outs)
        bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert bad.size == 0, f"stride {stride}: {bad.size} of {S} rows differ from their own launch, the first is row {bad[0]}"
    worst = 0.0
    for s in C.rot_model_streams(S):
        exact, bound = RM.rotate(x[s], states[s], C.ROT_BASE)
        err = np.abs(np.ascontiguousarray(want[s]).view(np.complex64).reshape(n).astype(np.complex128) - exact)
        assert (err <= bound).all(), (s, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    assert R.host_state(d_state).tobytes() == recs.tobytes(), "the rotation wrote a record"
    print(f"rotator rows: S {S}, n {n}, strides {n} and {n + 1}: 2 x {S} rows of {S} distinct records compared; 8 rows against float64, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("S", C.CONTROL_S)
def test_rotator_control(S):
    """records, d_applied and d_delta equal the Python-int model with max_slots = total and total - 5 (the last streams are cut), with
    and without the fine arrays; a stream that is not steered keeps its 32 bytes, `reserved` stays, the words behind d_applied[S - 1] and
    d_delta[S - 1] keep the sentinel"""
    import torch
    c = C.control_case(S)
    before = RM.to_records(c.before, ROTATOR_STATE)
    d = [R.dev(a) for a in c.arrays]
    d_off = R.dev(np.array(c.offsets, np.int32))
    steered = set()
    for max_slots in (c.total, c.total - C.CONTROL_CUT):
        for fine in (True, False):
            want_applied, want_delta, want_after = C.control_model(S, max_slots, fine)
            d_state = R.dev_state(before)
            d_applied = torch.full((S + 8,), -7, dtype=torch.int32, device="cuda")
            d_delta = torch.full((S + 8,), -7, dtype=torch.int64, device="cuda")
            rotator_control_device(d_off.data_ptr(), S, max_slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr() if fine else 0,
                                   d[4].data_ptr() if fine else 0, C.COARSE_SCALE, C.FINE_SCALE, C.CONTROL_AT, d_state.data_ptr(), d_applied.data_ptr(),
                                   d_delta.data_ptr(), 0, T.stream())
            torch.cuda.synchronize()
            after, applied, delta = R.host_state(d_state), d_applied.cpu().numpy(), d_delta.cpu().numpy()
            what = f"max_slots {max_slots} of {c.total}, fine {fine}"
            assert (applied[S:] == -7).all() and (delta[S:] == -7).all(), f"{what}: a write behind d_applied or d_delta"
            assert applied[:S].tolist() == want_applied, f"{what}: d_applied differs first at stream {np.flatnonzero(applied[:S] != np.array(want_applied))[0]}"
            assert delta[:S].tolist() == want_delta, what
            for s in range(S):
                assert after[s].tobytes() == want_after[s].tobytes(), f"{what}: record {s} is {after[s]}, the model's {want_after[s]}"
                if want_applied[s] <= 0:
                    assert after[s].tobytes() == before[s].tobytes()
                else:
                    assert int(after[s]["index"]) == C.CONTROL_AT and int(after[s]["reserved"]) == c.before[s]["reserved"]
                    steered.add(s)
    print(f"rotator control: S {S}, {len(set(c.variant.tolist()))} variants, {c.total} slots, 4 x {S} records compared, {len(steered)} streams steered, "
          f"{sum(1 for s in steered if s >= 256)} of them from stream 256 on")
    assert len(steered) > S // 4


# ------------------------------------------------------------------ 3. de-header rows
@pytest.mark.parametrize("S", C.DH_S)
def test_deheader_rows(S):
    """two calls, every stream cut at a point of its own: per call pkt_offsets, every stream's TS bytes and the canonical records are
    the oracle's, a stream without frames keeps its record bytes, the counters are the model's, and the guards of Rows.call hold; 16
    streams, the edges and the 300-frame stream among them, also equal a single BbDeheader fed the same frames in the same two calls"""
    c, model = C.dh_case(S), C.dh_model(S)
    max_frames = max(sum(len(f) for f in piece) for piece in c.pieces) + 3
    rows = D.Rows(C.KBCH, S, max_frames)
    singles = {s: BbDeheader(kbch_bits=C.KBCH, max_frames=C.DH_LONG_FRAMES) for s in C.dh_single_streams(S)}
    packets = 0
    for k, piece in enumerate(c.pieces):
        before = rows.records()
        got, pko = rows.call(piece)
        want = model[k]
        assert pko == want.pko, f"call {k}: pkt_offsets differ first at stream {np.flatnonzero(np.array(pko) != np.array(want.pko))[0]}"
        after = rows.records()
        for s in range(S):
            D.same_stream(got[s], want.out[s], f"call {k}, stream {s}")
            if len(piece[s]) == 0:
                assert after[s].tobytes() == before[s].tobytes(), f"call {k}: stream {s} got no frame and its record changed"
        assert BM.canon(after).tobytes() == BM.canon(want.records).tobytes(), k
        assert bbdeheader_state_counters(after) == want.counters, k
        for s, one in singles.items():
            if len(piece[s]):
                D.same_stream(got[s], one.work(piece[s]), f"call {k}, stream {s} against a single handle")
            assert one.counters() == want.counters[s], (k, s)
        packets += pko[-1]
    for one in singles.values():
        one.close()
    print(f"de-header rows: S {S}, {len(set(c.variant.tolist()))} variants, {sum(len(f) for f in c.frames)} frames in two calls, {packets} packets and "
          f"2 x {S} records compared, {len(singles)} streams against single handles")
    assert packets > 4 * S
