"""The straight-line trip of the class-8 run loop (csrc/ldpc_kernel.hpp, kRun): a run is entered only outside a frame's first sweep (that
sweep takes the layer loop's packed arm), it never holds the table's last layer (the record fetched ahead is a running pointer that must
not step past the table), its end is tested on the prefetched header against the run's first one, and each half of the loop unrolled by
two has the layer's barrier on its way. Bit for bit against the reference decoder (the genuine one in oracle/_ref where it was built,
else the plain-C restatement) on decoded LLRs, packed bits and return values, all four builds of the class forced (the two without
packed nodes compile the layer loop as it was and stand for "nothing else moved").

What can go wrong is decided by how runs and barriers fall, so the shapes are asserted on the CPU from the schedule (the barrier rule of
csrc/ldpc_schedule.cpp restated from the layers' groups), over the tables together:
  runs of length 1, 2 and 3; a run that ends at a hazard layer, one that ends at the wrap to layer 0, one that ends at a degree change;
  a barrier layer as the first and as the second trip of the unrolled pair, and two barrier-free trips in a row.
Three frames (odd: a workgroup of its own in the one-frame builds, a half-empty pair in the others), group sizes 1 and 32, update caps 1
(the first sweep alone: no run is entered), 2 (the first sweep that loads messages: the first one through the runs) and 5; noise, zeros,
codewords near the threshold, and saturating input drawn from {-128, 127}: -128 is the byte whose magnitude saturates in the packed form."""
import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import LdpcDecoder, capi, ldpc_layer_info, ldpc_table_info
from test_class8_builds_gpu import BUILDS
from test_class8_run_loop_gpu import check, force, reference

NF = 3
TABLES = ["S2_TABLE_B4", "S2_TABLE_C3", "S2X_TABLE_B11", "S2_TABLE_C4"]
KINDS = ["noise", "zero", "near_threshold", "saturating"]
CAPS = [1, 2, 5]
GROUPS = [1, 32]


def schedule(table):
    """per layer: (regular, degree, barrier in front of it) -- the barrier rule of ldpc_schedule.cpp: layer 0, a hazard layer, or a layer
    that touches a bit group some layer behind the last barrier has touched (layer 0 and the last layer share the last parity group)"""
    info = ldpc_table_info(table)
    q, last_parity = info["q"], info["N"] // 360 - 1
    out, epoch = [], set()
    for i in range(q):
        li = ldpc_layer_info(table, i)
        mine = set(li["groups"])
        if i in (0, q - 1):
            mine.add(last_parity)
        hit = i == 0 or li["block"] < 360 or bool(mine & epoch)
        if hit:
            epoch = set()
        epoch |= mine
        out.append((i > 0 and li["block"] == 360, li["cnt"] + 2, hit))
    return out


def runs(table):
    """[(length, how it ends, barrier flags of its layers)] of the maximal stretches of regular layers of one degree"""
    s = schedule(table)
    q, out, i = len(s), [], 0
    while i < q:
        if not s[i][0]:
            i += 1
            continue
        j = i
        while j + 1 < q and s[j + 1][0] and s[j + 1][1] == s[i][1]:
            j += 1
        end = "wrap" if j == q - 1 else "degree" if s[j + 1][0] else "hazard"
        out.append((j - i + 1, end, [s[k][2] for k in range(i, j + 1)]))
        i = j + 1
    return out


def test_tables_cover_the_trip_shapes():
    allruns = [r for t in TABLES for r in runs(t)]
    for t in TABLES:
        deg = max(d for _, d, _ in schedule(t))
        assert 4 < deg <= 8, f"{t} is not a table of the degree class 8"
    for n in (1, 2, 3):
        assert any(r[0] == n for r in allruns), f"no regular run of length {n}"
    for end in ("hazard", "wrap", "degree"):
        assert any(r[1] == end for r in allruns), f"no regular run that ends at: {end}"
    # the trips of a run alternate between the halves of the unrolled pair, the run's first layer in the first half
    assert any(b for r in allruns for b in r[2][0::2]), "no barrier layer as the first trip of a pair"
    assert any(b for r in allruns for b in r[2][1::2]), "no barrier layer as the second trip of a pair"
    assert any(not a and not b for r in allruns for a, b in zip(r[2], r[2][1:])), "no two barrier-free trips in a row"
    # the benchmark's table alone has every barrier shape and a run that reaches the last layer
    b4 = runs("S2_TABLE_B4")
    assert any(b for r in b4 for b in r[2][0::2]) and any(b for r in b4 for b in r[2][1::2]) and any(r[1] == "wrap" for r in b4)


def make(table, kind):
    N = T.ldpc_info(table)[0]
    if kind == "noise":
        return T.llr_noise(NF, N, seed=41)
    if kind == "saturating":  # both ends of the byte range: -128 has no int8 magnitude
        return np.random.default_rng(42).choice(np.array([-128, 127], np.int8), (NF, N))
    if kind == "zero":
        return np.zeros((NF, N), np.int8)
    # codewords at amplitude 6, sigma below, near and above what five updates repair
    clean, _ = T.llr_codeword_awgn(table, NF, 43, amp=6.0, sigma=0.0)
    sigma = np.array([2.5, 4.0, 7.0])[:, None]
    noise = np.random.default_rng(44).normal(0.0, 1.0, clean.shape)
    return np.clip(np.rint(clean.astype(np.float64) + sigma * noise), -128, 127).astype(np.int8)


_want = {}


def expected(table, kind, G, cap):
    key = (table, kind, G, cap)
    if key not in _want:
        llr = make(table, kind)
        _want[key] = (llr,) + reference(table, llr, G, cap)
    return _want[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("table", TABLES)
def test_trip_vs_reference(table, build, kind, monkeypatch):
    kernel = force(monkeypatch, build)
    N, K, _, _ = T.ldpc_info(table)
    for G in GROUPS:
        dec = LdpcDecoder(table=table, message_bits=K, group_size=G, max_frames=NF, max_trials=CAPS[0], outputmode=capi.OM_CODEWORD)
        assert dec.kernel_name == kernel
        for cap in CAPS:
            dec.max_trials = cap
            llr, want, wret = expected(table, kind, G, cap)
            check(dec, llr, want, wret, N, (table, build, G, cap, kind))
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_trip_resumed_frame(build, monkeypatch):
    """A frame stopped after two updates and continued to five by a resume launch of the handle: frame 0 passes its test after two
    updates (asserted against the restatement), gives up waiting for its group at once (DVBS2_GROUP_SPIN_MAX=0) and is taken up again
    by the handle's resume launches, because frames 1 (noise) and 2 (saturating bytes) keep the group running to the cap. A resumed sweep
    starts with messages in memory and an update count above zero: straight into the first run, with no first sweep in front of it."""
    table = "S2_TABLE_B4"
    kernel = force(monkeypatch, build)
    monkeypatch.setenv("DVBS2_GROUP_SPIN_MAX", "0")
    monkeypatch.setenv("DVBS2_RESOLVE_ROUNDS", "2")
    N, K, _, _ = T.ldpc_info(table)
    llr, _ = T.llr_codeword_awgn(table, NF, 31, amp=6.0, sigma=2.5)
    llr[1] = T.llr_noise(1, N, 32)[0]
    llr[2] = np.random.default_rng(45).choice(np.array([-128, 127], np.int8), N)
    assert T.oracle_ldpc_decode(table, llr[:1], 1, 5)[1] == [3], "frame 0 alone must stop after exactly two of five updates"
    want, wret = reference(table, llr, 32, 5)
    assert wret == [-1]
    dec = LdpcDecoder(table=table, message_bits=K, group_size=32, max_frames=NF, max_trials=5, outputmode=capi.OM_CODEWORD)
    assert dec.kernel_name == kernel
    check(dec, llr, want, wret, N, (table, build, "resume"))
    dec.close()
