"""The run loop's trip fetches the next layer's wave record from INSIDE the packed node, behind its input phase (csrc/ldpc_kernel.hpp,
DVBS2_RUN_TRIP; the hook of check_node_v2<.., RUN> in csrc/ldpc_node_packed.hpp), so that the node's first LDS wait no longer covers
scalar loads. What can go wrong there: a trip working on a record set the hook has already overwritten (the sets are ping-pong), a run
handing the layer loop a record or messages that are not the next layer's at either of its two exits, a run's first trip taking a record
that the layer loop held in other registers, the wrap select reading a mask that is not the trip's. Every case is bit for bit against the
reference decoder (the genuine one in oracle/_ref where it was built, else the plain-C restatement) on decoded LLRs, packed bits and
return values.

Builds and tables: the four class-8 builds forced on 1/2 normal (B4), 2/5 normal (B3), S2X 9/20 (B11), 2/5 short (C3) and 1/2 short (C4);
<4, packed, solo> on 1/4 normal (B1). tests/test_class8_trip_gpu.py asserts that these tables hold runs of length 1, 2 and 3, runs ending at a
hazard layer, at a degree change and in front of the last layer, and barrier layers as the first and as the second trip of a pair. Shapes:
three frames in groups of one, 33 frames in groups of 32. Caps 1 (never enters a run), 2 and 3 (the first entries into a run, behind a
first sweep that loaded nothing) and 5. Inputs: noise, all zero, bytes from {-128, 127}, codewords that converge inside the cap, a resumed
frame. One case per build runs the group stop as host-driven rounds (DVBS2_GROUP_SYNC=0): a second launch continues from the messages a
first launch stored.

The inputs are those of tests/test_class8_parity_carry_gpu.py, whose cache of reference results is shared: a reference is computed once."""
import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import LdpcDecoder, capi
from test_class8_builds_gpu import BUILDS
from test_class8_run_loop_gpu import check, force, reference
from test_class8_parity_carry_gpu import expected

TABLES = ["S2_TABLE_B4", "S2_TABLE_B3", "S2X_TABLE_B11", "S2_TABLE_C3", "S2_TABLE_C4"]
CLASS4 = ("S2_TABLE_B1", "ldpc_layered_kernel<4, packed, solo>")
KINDS = ["noise", "zero", "saturating", "near_threshold"]  # (saturating: bytes from {-128, 127}; near_threshold: codewords that converge inside the cap)
CAPS = [1, 2, 3, 5]
SHAPES = [(3, 1), (33, 32)]  # (frames, group size)


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
def test_trip_waits_vs_reference(table, build, kind, monkeypatch):
    kernel = force(monkeypatch, build)
    run_case(table, kernel, kind, (table, build, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_trip_waits_class4_vs_reference(kind, monkeypatch):
    force(monkeypatch, "packed-solo")
    run_case(CLASS4[0], CLASS4[1], kind, (CLASS4[0], "packed-solo", kind))


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_trip_waits_resumed_frame(build, monkeypatch):
    """A frame stopped after two updates and continued to five by a resume launch of the handle: frame 0 passes its test after two updates,
    gives up waiting for its group at once and is taken up again by the handle's resume launches, because frames 1 (noise) and 2 (bytes
    from {-128, 127}) keep the group running to the cap. The resumed sweep enters its first run with messages in memory."""
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
def test_trip_waits_host_driven_rounds(build, monkeypatch):
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
