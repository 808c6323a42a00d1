"""CPU: the conditions on the inputs of tests/test_many_streams_gpu.py, asserted from the assignments and the models alone
(tests/many_streams_case.py). They are what makes a wrong stream index visible there: neighbours at the lags of the kernels' strides
carry other variants, the streams at the edges of the kernels' chunks carry data, every block of 64 streams of the de-header rows moves
packets, and every outcome of the control rule occurs on both sides of the first workgroup."""
import numpy as np
import pytest

import many_streams_case as C


def check_lags(variant, what):
    shares = C.lag_shares(variant)
    print(f"{what}: {len(set(np.asarray(variant).tolist()))} variants; share of streams that differ from the one `lag` before: "
          + ", ".join(f"{d}: {v:.3f}" for d, v in shares.items()))
    assert shares and all(v >= C.LAG_SHARE for v in shares.values()), (what, shares)


def test_edges():
    assert C.edges(17) == [0, 15, 16] and C.edges(256) == [0, 15, 16, 17, 255]
    assert C.edges(257) == [0, 15, 16, 17, 255, 256] and C.edges(1024) == [0, 15, 16, 17, 255, 256, 257, 1023]


# ------------------------------------------------------------------ 1. search, gather, coarse estimate
@pytest.mark.parametrize("S", C.PL_S)
def test_pl_assignment(S):
    v = C.pl_assignment(S)
    assert len(v) == S and 0 <= v.min() and v.max() < 13
    check_lags(v, f"PL, S {S}")
    # the edges are trimmed or untrimmed CLEAN streams; that these lock and have selected records is asserted from the single-stream
    # references where the device is (test_many_streams_gpu.test_pl_references)
    assert all(int(v[e]) in C.PL_PRODUCTIVE for e in C.edges(S))
    assert len(C.PL_PRODUCTIVE) == 6 and all(C.PL_VARIANTS[p][0] in (C.B.CLEAN_A, C.B.CLEAN_B) for p in C.PL_PRODUCTIVE)
    if S >= 257:
        assert len(set(v.tolist())) == 13
    start = C.pl_start_calls(S)
    assert len(start) == S and set(start) == {0, 1, 2}
    for p in set(v.tolist()):  # streams of one variant do not move in lockstep
        if np.count_nonzero(v == p) >= 8:
            assert len({start[s] for s in np.flatnonzero(v == p)}) > 1, p


# ------------------------------------------------------------------ 2. rotator rows and control
@pytest.mark.parametrize("S", C.ROT_S)
def test_rotator_records(S):
    st = C.rot_records(S)
    assert (st[0]["inc"], st[256 if S > 257 else 255]["inc"], st[S - 1]["inc"]) == (0, 1 << 63, (1 << 64) - 1)
    assert len({(r["phase"], r["inc"], r["index"]) for r in st}) == S
    assert any(r["index"] < 0 for r in st) and any(r["index"] > C.ROT_BASE + 513 for r in st)
    pick = C.rot_model_streams(S)
    assert len(pick) == 8 and {0, 255, 256, S - 1} <= set(pick)
    for n in C.ROT_N:
        x = C.rot_input(S, n)
        assert x.shape == (S, n) and x.dtype == np.complex64


@pytest.mark.parametrize("S", C.CONTROL_S)
def test_control_case(S):
    c = C.control_case(S)
    check_lags(c.variant, f"control, S {S}")
    assert len(c.offsets) == S + 1 and c.total == c.offsets[-1] > C.CONTROL_CUT
    assert set(np.diff(c.offsets).tolist()) == {0, 1, 2, 3, 4}
    applied, delta, after = C.control_model(S, c.total, True)
    before = C.RM.to_records(c.before, C.ROTATOR_STATE)
    for e in C.edges(S):  # the edge streams are steered
        assert applied[e] in (1, 2) and after[e].tobytes() != before[e].tobytes(), e
    kinds = {k: {a for a in applied[lo:hi]} for k, (lo, hi) in (("below 256", (0, 256)), ("from 256", (256, S)))}
    print(f"control, S {S}: applied {[applied.count(k) for k in (-1, 0, 1, 2)]} of kinds -1, 0, 1, 2; from stream 256 on {sorted(kinds['from 256'])}")
    assert kinds["below 256"] == {-1, 0, 1, 2}
    if S == 1024:
        assert kinds["from 256"] == {-1, 0, 1, 2}
    # with max_slots CONTROL_CUT below the total the last streams are cut: the outcome of at least one changes
    cut = C.control_model(S, c.total - C.CONTROL_CUT, True)
    assert cut[0] != applied and cut[0][:S - 8] == applied[:S - 8]
    # without the fine arrays no fine step is taken, and some stream that took one falls back to its coarse estimate or to nothing
    nofine = C.control_model(S, c.total, False)
    assert 2 not in nofine[0] and 2 in applied and nofine[0] != applied


# ------------------------------------------------------------------ 3. de-header rows
@pytest.mark.parametrize("S", C.DH_S)
def test_deheader_case(S):
    c, m = C.dh_case(S), C.dh_model(S)
    check_lags(c.variant, f"de-header, S {S}")
    n1, n2 = ([len(p) for p in piece] for piece in c.pieces)
    assert len(c.frames[c.long]) == 300 and 0 < c.cut[c.long] < 300 and (c.long >= 256 or S == 256)
    assert all(0 <= len(f) <= 6 for s, f in enumerate(c.frames) if s != c.long) and {len(f) for f in c.frames} >= set(range(7))
    assert n1.count(0) > S // 16 and n2.count(0) > S // 16  # streams without a frame in one of the calls
    assert sum(1 for a, b in zip(n1, n2) if a and b) > S // 4  # streams whose partial packet and record cross the call
    assert len({f.tobytes() for f in c.frames if len(f)}) == sum(1 for f in c.frames if len(f)), "two streams carry the same bytes"
    pk = [np.diff(call.pko) for call in m]
    print(f"de-header, S {S}: frames per call {sum(n1)}, {sum(n2)}; packets per call {int(pk[0].sum())}, {int(pk[1].sum())}")
    for e in C.edges(S):
        assert pk[0][e] > 0, f"edge stream {e} has no packet in the first call"
    # every block of 64 consecutive streams: at least half yield a packet in the first call, so a wrong partial sum at any wavefront
    # boundary of the prefix scan moves a non-empty stream's packets
    for b in range(0, S - 63):
        assert np.count_nonzero(pk[0][b:b + 64]) >= 32, (b, int(np.count_nonzero(pk[0][b:b + 64])))
    # the fuzzed share meets everything the block reacts to, among the streams from 256 on
    if S > 256:
        counters = m[1].counters[256:]
        for k in ("dropped", "gaps", "errors"):
            assert sum(r[k] for r in counters) > 0, k
    if S == 1024:  # ... and without the long stream
        counters = [r for s, r in enumerate(m[1].counters) if s >= 256 and s != c.long]
        for k in ("dropped", "gaps", "errors"):
            assert sum(r[k] for r in counters) > 0, k
    pick = C.dh_single_streams(S)
    assert len(pick) == C.DH_SINGLES and set(C.edges(S)) <= set(pick) and c.long in pick
