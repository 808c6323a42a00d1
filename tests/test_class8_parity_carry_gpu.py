"""The run-loop form of the packed check node (csrc/ldpc_node_packed.hpp, check_node_v2<.., RUN>; kRun in csrc/ldpc_kernel.hpp): inside a
run of regular packed layers the own-parity LLR of a trip stays in a register and is the next trip's previous-parity input (loaded in
front of a run's first trip, written to LDS behind its last one) and the wrap fix of an address is a select of its base on the record's
lane mask (no EXEC change); the class-8 builds keep a row's two message words as one 8-byte record. Results stay bit for bit: every GPU case is compared with the reference decoder (the genuine one in oracle/_ref where it was built, else the plain-C restatement) on decoded LLRs, packed
bits and return values.

Builds and tables: the four class-8 builds forced on 1/2 normal (B4, the benchmark's table), 2/5 normal, S2X 9/20 normal, 2/5 short and
1/2 short; <4, packed, solo> on 1/4 normal. Shapes: three frames in groups of one (two share a CU, one is alone) and 33 frames in groups
of 32 (one full group and a tail). Caps 1 (never enters a run), 2 and 3 (one and two sweeps through the runs: what a run left in LDS is read by a
syndrome test and by another sweep; runs of odd and of even length are in the tables, tests/test_class8_trip_gpu.py asserts it) and 5. Inputs: noise; all zero; bytes from {-128, 127} only (-128 is the half whose magnitude saturates: 0x8000 must
come out 0x7fff); codewords in noise that converge inside the cap, so that the full syndrome test reads what the runs left in LDS; a
resumed frame. One case per build switches the group stop to host-driven rounds (DVBS2_GROUP_SYNC=0): a second launch then continues
from the messages a first launch stored (the case that catches a mismatch of the message layout between paths).

CPU: for all 57 tables and every packed build the planner gives them, what the carry relies on in the (layer, wave) records -- in every
packed regular record of a layer 0 < i < q - 1 (each can be a trip of a run, if only of a run of one trip) the two parity slots lie 360
bytes apart and neither is a fix slot, and where a run can pass from one record to the next, the previous-parity slot of the second names
the byte of the own-parity slot of the first --, from the planner's host entry (tests/ldpc_plan_main.cpp). (The issue's fourth step, the
sign mask taken once per pair, measured slower and is not in the tree, so it has no test: notes/r11_parity_carry.md.)"""
import re
import subprocess

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import LdpcDecoder, capi
from test_class8_builds_gpu import BUILDS
from test_class8_run_loop_gpu import check, force, reference

TABLES = ["S2_TABLE_B4", "S2_TABLE_B3", "S2X_TABLE_B11", "S2_TABLE_C3", "S2_TABLE_C4"]
CLASS4 = ("S2_TABLE_B1", "ldpc_layered_kernel<4, packed, solo>")
KINDS = ["noise", "zero", "saturating", "near_threshold"]
CAPS = [1, 2, 3, 5]
SHAPES = [(3, 1), (33, 32)]  # (frames, group size)


# ---- CPU: the records the parity carry relies on --------------------------------------------------------------------------------

PACKED_SETS = [T.VARIANTS["packed-pair"], T.VARIANTS["packed-solo"], T.VARIANTS["soft-barrier"], T.VARIANTS["policy"], T.VARIANTS["classic"]]
K_PACKED, K_BLOCK_SHIFT = 1 << 13, 16  # csrc/ldpc_layout.h: kRecPacked, kRecBlockShift


def planner_wrecs(exe, rows):
    """[(kernel name, dmax, wave records as a (q, 6, RSW) array) or (error text, 0, None)] -- the protocol of tests/ldpc_plan_main.cpp"""
    text = "".join("%s 32 %s\n" % (t, " ".join("%s=%s" % kv for kv in sorted(env.items()))) for t, env in rows)
    r = subprocess.run([exe], input=text.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr
    out, pos, plans = r.stdout, 0, []
    while pos < len(out):
        end = out.index(b"\n", pos)
        kind, f = out[pos:pos + 1], out[pos + 2:end].decode().split("|")
        pos = end + 1
        if kind == b"E":
            plans.append((f[0], 0, None))
            continue
        dmax, n_recs, n_wrecs = int(f[1]), int(f[6]), int(f[7])
        w = np.frombuffer(out, np.uint32, n_wrecs, pos + 4 * n_recs)
        pos += 4 * (n_recs + n_wrecs)
        plans.append((f[0], dmax, w.reshape(-1, 6, 2 * dmax + 12)))
    assert len(plans) == len(rows)
    return plans


def test_parity_slots_of_consecutive_packed_records(tmp_path):
    exe = T.build_ldpc_planner(tmp_path)
    text = open(T.ROOT + "/gr-dvbs2rx_amd/csrc/ldpc_policy.inc").read()
    tables = sorted(set(re.findall(r'\{ "(\w+)", \d, \d \}', text)))
    assert len(tables) == 57
    rows = [(t, env) for t in tables for env in PACKED_SETS]
    seen, records, pairs, lone, class8 = set(), 0, 0, {}, set()
    for (table, env), (name, dmax, wr) in zip(rows, planner_wrecs(exe, rows)):
        assert wr is not None, (table, env, name)
        if not (name.startswith("ldpc_layered_kernel<") and "packed" in name) or (table, name) in seen:
            continue
        seen.add((table, name))
        q = wr.shape[0]
        nfix = 10 if dmax == 32 else dmax // 4
        key = lambda h: (int(h) >> K_BLOCK_SHIFT, int(h) & K_PACKED, int(h) & 0xff)  # what a run's records share: block, format, degree
        eligible = lambda i, w: 0 < i < q - 1 and bool(int(wr[i, w][0]) & K_PACKED) and (int(wr[i, w][0]) >> K_BLOCK_SHIFT) >= 360
        for i in range(1, q - 1):
            for w in range(6):
                if not eligible(i, w):
                    continue  # the run loop takes every other record of these layers, if only for a run of one trip
                a = wr[i, w]
                own = int(a[0]) & 0xff  # the slots behind the data entries: own parity, then previous parity
                what = (table, name, i, w)
                assert int(a[4 + own]) == int(a[4 + own + 1]) + 360, what
                for slot in (own, own + 1):
                    assert slot >= nfix or not (int(a[4 + dmax + 2 * slot]) | int(a[4 + dmax + 2 * slot + 1])), what
                records += 1
                follows = eligible(i - 1, w) and key(wr[i - 1, w][0]) == key(a[0])
                followed = eligible(i + 1, w) and key(wr[i + 1, w][0]) == key(a[0])
                if followed:  # two consecutive trips of a run: the second takes its previous parity from the carry
                    assert int(wr[i + 1, w][4 + own + 1]) == int(a[4 + own]), what
                    pairs += 1
                if not follows and not followed:
                    lone[table] = lone.get(table, 0) + 1
                if dmax <= 8:
                    class8.add(table)
    assert records > pairs > 1000 and {"S2_TABLE_B4", "S2_TABLE_B3", "S2X_TABLE_B11", "S2_TABLE_C3", "S2_TABLE_C4", "S2_TABLE_B1"} <= class8, (records, pairs, class8)
    # runs of ONE trip (no neighbour of the same key on either side) are among what was checked: most of 1/2 short is such records
    assert {"S2_TABLE_C4", "S2_TABLE_C3", "S2_TABLE_B3"} <= set(lone) and lone["S2_TABLE_C4"] >= 50, lone


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def make(table, kind, nf):
    N = T.ldpc_info(table)[0]
    if kind == "noise":
        return T.llr_noise(nf, N, seed=61)
    if kind == "zero":
        return np.zeros((nf, N), np.int8)
    if kind == "saturating":
        return np.random.default_rng(62).choice(np.array([-128, 127], np.int8), (nf, N))
    # codewords at amplitude 6: the first frames converge within two or three updates, the last ones not within five
    clean, _ = T.llr_codeword_awgn(table, nf, 63, amp=6.0, sigma=0.0)
    sigma = np.linspace(2.0, 7.0, nf)[:, None]
    noise = np.random.default_rng(64).normal(0.0, 1.0, clean.shape)
    return np.clip(np.rint(clean.astype(np.float64) + sigma * noise), -128, 127).astype(np.int8)


_want = {}


def expected(table, kind, nf, G, cap):
    key = (table, kind, nf, G, cap)
    if key not in _want:
        llr = make(table, kind, nf)
        _want[key] = (llr,) + reference(table, llr, G, cap)
    return _want[key]


def run_case(table, kernel, kind, what):
    N, K, _, _ = T.ldpc_info(table)
    for nf, G in SHAPES:
        dec = LdpcDecoder(table=table, message_bits=K, group_size=G, max_frames=nf, max_trials=CAPS[0], outputmode=capi.OM_CODEWORD)
        assert dec.kernel_name == kernel
        for cap in CAPS:
            dec.max_trials = cap
            llr, want, wret = expected(table, kind, nf, G, cap)
            check(dec, llr, want, wret, N, what + (nf, G, cap))
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("table", TABLES)
def test_run_node_vs_reference(table, build, kind, monkeypatch):
    kernel = force(monkeypatch, build)
    run_case(table, kernel, kind, (table, build, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_run_node_class4_vs_reference(kind, monkeypatch):
    force(monkeypatch, "packed-solo")
    run_case(CLASS4[0], CLASS4[1], kind, (CLASS4[0], "packed-solo", kind))


def test_near_threshold_input_converges_inside_the_cap():
    """the input that makes the full syndrome test read the bytes a run left behind: some frame of B4 stops before the cap, some does not"""
    llr = make("S2_TABLE_B4", "near_threshold", 3)
    rets = [T.oracle_ldpc_decode("S2_TABLE_B4", llr[f:f + 1], 1, 5)[1][0] for f in range(3)]
    assert any(r >= 1 for r in rets) and any(r == -1 for r in rets), rets  # (updates left; -1: not within the cap)


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_run_node_resumed_frame(build, monkeypatch):
    """A frame stopped after two updates and continued to five by a resume launch of the handle (as tests/test_class8_trip_gpu.py): frame 0
    passes its test after two updates, gives up waiting for its group at once and is taken up again by the handle's resume launches,
    because frames 1 (noise) and 2 (bytes from {-128, 127}) keep the group running to the cap."""
    table = "S2_TABLE_B4"
    kernel = force(monkeypatch, build)
    monkeypatch.setenv("DVBS2_GROUP_SPIN_MAX", "0")
    monkeypatch.setenv("DVBS2_RESOLVE_ROUNDS", "2")
    N, K, _, _ = T.ldpc_info(table)
    llr, _ = T.llr_codeword_awgn(table, 3, 31, amp=6.0, sigma=2.5)
    llr[1] = T.llr_noise(1, N, 65)[0]
    llr[2] = np.random.default_rng(66).choice(np.array([-128, 127], np.int8), N)
    assert T.oracle_ldpc_decode(table, llr[:1], 1, 5)[1] == [3], "frame 0 alone must stop after exactly two of five updates"
    want, wret = reference(table, llr, 32, 5)
    assert wret == [-1]
    dec = LdpcDecoder(table=table, message_bits=K, group_size=32, max_frames=3, max_trials=5, outputmode=capi.OM_CODEWORD)
    assert dec.kernel_name == kernel
    check(dec, llr, want, wret, N, (table, build, "resume"))
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_run_node_host_driven_rounds(build, monkeypatch):
    """The group stop as host-driven rounds: frames stop at their own good point, the host resolves the groups and launches again, and a
    later launch continues from the messages an earlier one stored. 33 frames in groups of 32, codewords that stop at different counts."""
    table = "S2_TABLE_B4"
    kernel = force(monkeypatch, build)
    monkeypatch.setenv("DVBS2_GROUP_SYNC", "0")
    N, K, _, _ = T.ldpc_info(table)
    nf, G, cap = 33, 32, 5
    llr, want, wret = expected(table, "near_threshold", nf, G, cap)
    dec = LdpcDecoder(table=table, message_bits=K, group_size=G, max_frames=nf, max_trials=cap, outputmode=capi.OM_CODEWORD)
    assert dec.kernel_name == kernel
    check(dec, llr, want, wret, N, (table, build, "host-driven rounds"))
    dec.close()
