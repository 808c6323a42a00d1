"""The run loop of the degree class 8 (csrc/ldpc_kernel.hpp, kRun): the packed builds run every maximal stretch of regular packed layers
of one degree in a loop of its own, unrolled by two over ping-pong record and message registers. Bit for bit against the reference decoder
(the genuine one in oracle/_ref where it was built, else the plain-C restatement) on decoded LLRs, packed bits and return values, with all
four builds of the class forced (the two without packed nodes compile the layer loop as it was and stand for "nothing else moved").

What can go wrong is decided by how the runs fall, so the tables are chosen for that:
  S2_TABLE_B4    runs broken by single-pair chain layers, layer 0 in front of a run (the benchmark's table)
  S2_TABLE_C3    2/5 short: runs of length one next to hazard layers
  S2X_TABLE_B11  9/20 normal: no hazard layer, one run of degree 8 handing over to one of degree 7
  S2_TABLE_C4    short: a run of length one, a run of even length and a degree change between adjacent regular layers -- asserted below
                 from the schedule, so the table cannot silently stop covering them
Three frames (odd: a workgroup of its own in the one-frame builds, a half-empty pair in the others), group sizes 1 and 32, and update
caps 1 (a frame's first sweep only: zero messages, nothing loaded), 2 (the first sweep that loads messages) and 5."""
from itertools import groupby

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import LdpcDecoder, capi, ldpc_layer_info, ldpc_table_info
from test_class8_builds_gpu import BUILDS

NF = 3
TABLES = ["S2_TABLE_B4", "S2_TABLE_C3", "S2X_TABLE_B11", "S2_TABLE_C4"]
MIXED_RUNS_TABLE = "S2_TABLE_C4"
KINDS = ["noise", "near_threshold", "saturating", "zero"]
CAPS = [1, 2, 5]
GROUPS = [1, 32]


def regular_runs(table):
    """[(degree, length)] of the maximal stretches of regular layers (not layer 0, no hazard) of one degree, and whether two such
    stretches of different degree are adjacent"""
    q = ldpc_table_info(table)["q"]
    key = []
    for i in range(q):
        li = ldpc_layer_info(table, i)
        key.append((li["cnt"] + 2, -1) if i > 0 and li["block"] == 360 else (None, i))
    runs = [(k[0], len(list(g))) for k, g in groupby(key)]
    adjacent = any(a[0] is not None and b[0] is not None for a, b in zip(runs, runs[1:]))
    return [r for r in runs if r[0] is not None], adjacent


def test_tables_cover_the_run_shapes():
    runs, adjacent = regular_runs(MIXED_RUNS_TABLE)
    assert max(d for d, _ in runs) <= 8 and max(d for d, _ in runs) > 4, "not a table of the degree class 8"
    assert any(n == 1 for _, n in runs), "no regular run of length one"
    assert any(n % 2 == 0 for _, n in runs), "no regular run of even length"
    assert adjacent, "no degree change between adjacent regular layers"
    assert len(regular_runs("S2_TABLE_B4")[0]) > 1, "B4's runs are no longer broken by hazard layers"


def make(table, kind):
    N = T.ldpc_info(table)[0]
    if kind == "noise":
        return T.llr_noise(NF, N, seed=21)
    if kind == "saturating":  # +-127 only
        return np.random.default_rng(22).choice(np.array([-127, 127], np.int8), (NF, N))
    if kind == "zero":
        return np.zeros((NF, N), np.int8)
    # codewords at amplitude 6, sigma below, near and above what five updates repair
    clean, _ = T.llr_codeword_awgn(table, NF, 23, amp=6.0, sigma=0.0)
    sigma = np.array([2.5, 4.0, 7.0])[:, None]
    noise = np.random.default_rng(24).normal(0.0, 1.0, clean.shape)
    return np.clip(np.rint(clean.astype(np.float64) + sigma * noise), -128, 127).astype(np.int8)


_pad = {}


def reference(table, llr, G, trials):
    """Groups of G frames (the last one partial) through the reference. The genuine decoder works on batches of 32: a group is filled up
    with clean codewords, which pass every syndrome test and so never change when their batch stops."""
    if T.ref_ldpc() is None:
        outs, rets = [], []
        for g in range(0, llr.shape[0], G):
            o, r = T.oracle_ldpc_decode(table, llr[g:g + G], llr[g:g + G].shape[0], trials)
            outs.append(o); rets += list(r)
        return np.concatenate(outs), rets
    if table not in _pad:
        _pad[table] = T.make_input(table, "clean", 32, seed=25)
    outs, rets = [], []
    for g in range(0, llr.shape[0], G):
        part = llr[g:g + G]
        batch = np.concatenate([part, _pad[table][:32 - part.shape[0]]])
        o, r = T.ref_ldpc_decode(table, batch, 0, trials)
        outs.append(o[:part.shape[0]]); rets += list(r)
    return np.concatenate(outs), rets


_want = {}


def expected(table, kind, G, cap):
    key = (table, kind, G, cap)
    if key not in _want:
        llr = make(table, kind)
        _want[key] = (llr,) + reference(table, llr, G, cap)
    return _want[key]


def force(monkeypatch, build):
    v2, solo, kernel = BUILDS[build]
    for k, v in {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": v2, "DVBS2_SOLO": solo}.items():
        monkeypatch.setenv(k, v)
    return kernel


def check(dec, llr, want, wret, N, what):
    bits, out, ret = dec.work(llr, want_llr=True)
    assert ret.tolist() == wret, what
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: LLR mismatch in frames {bad}"
    assert np.array_equal(bits, T.pack_bits(want, N)), what


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("table", TABLES)
def test_run_loop_vs_reference(table, build, monkeypatch):
    kernel = force(monkeypatch, build)
    N, K, _, _ = T.ldpc_info(table)
    for G in GROUPS:
        dec = LdpcDecoder(table=table, message_bits=K, group_size=G, max_frames=NF, max_trials=CAPS[0], outputmode=capi.OM_CODEWORD)
        assert dec.kernel_name == kernel
        for cap in CAPS:
            dec.max_trials = cap
            for kind in KINDS:
                llr, want, wret = expected(table, kind, G, cap)
                check(dec, llr, want, wret, N, (table, build, G, cap, kind))
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_run_loop_resumed_frame(build, monkeypatch):
    """A frame stopped after two updates and continued to five by a resume launch of the handle: frame 0 passes its test after two
    updates (asserted against the restatement), gives up waiting for its group at once (DVBS2_GROUP_SPIN_MAX=0) and is taken up again
    by the handle's resume launches, because frame 1 (noise) keeps the group running to the cap. A resumed sweep starts with messages
    in memory and an update count above zero, into the first run."""
    table = "S2_TABLE_B4"
    kernel = force(monkeypatch, build)
    monkeypatch.setenv("DVBS2_GROUP_SPIN_MAX", "0")
    monkeypatch.setenv("DVBS2_RESOLVE_ROUNDS", "2")
    N, K, _, _ = T.ldpc_info(table)
    llr, _ = T.llr_codeword_awgn(table, NF, 31, amp=6.0, sigma=2.5)
    llr[1] = T.llr_noise(1, N, 32)[0]
    assert T.oracle_ldpc_decode(table, llr[:1], 1, 5)[1] == [3], "frame 0 alone must stop after exactly two of five updates"
    want, wret = reference(table, llr, 32, 5)
    assert wret == [-1]
    dec = LdpcDecoder(table=table, message_bits=K, group_size=32, max_frames=NF, max_trials=5, outputmode=capi.OM_CODEWORD)
    assert dec.kernel_name == kernel
    check(dec, llr, want, wret, N, (table, build, "resume"))
    dec.close()
