"""Every build of the degree class 8 (plain, packed, one-frame, packed one-frame), forced on three tables, bit-exact against the genuine
reference decoder in oracle/_ref (the plain-C restatement where that was not built) on decoded LLRs, packed bits and return values.

The four builds share one translation unit and the layer loop around their check nodes (message hand-over between layers, the zero
messages of a frame's first sweep, the degree switch), and the packed builds share the single-pair lane-chain node of the hazard layers:
  S2_TABLE_B4    QPSK 1/2 normal, the benchmark's table: eight hazard layers, all of them single-pair lane chains
  S2_TABLE_C3    2/5 short: eight hazard layers (blocks 12 .. 169: lane chains and the block scheme), degrees 6 and 7
  S2X_TABLE_B11  9/20 normal. No S2X table of this degree class has a hazard layer (tools/dump_hazards.cc: B2, B3, B11, C2, C3, C10
                 all report none), so this one stands for the regular layers of a table whose default build is the packed one-frame one.
Inputs: saturating LLRs; codewords in noise whose level rises over the frames of the batch from well below to well above the decoding
threshold, so that frames stop at many different update counts and some never do; and pure noise, which never converges (the
benchmark's input)."""
import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import LdpcDecoder, capi

pytestmark = pytest.mark.gpu

G = 32
TRIALS = 16
TABLES = ["S2_TABLE_B4", "S2_TABLE_C3", "S2X_TABLE_B11"]
BUILDS = {  # forced build -> (DVBS2_V2, DVBS2_SOLO, kernel)
    "plain": ("0", "0", "ldpc_layered_kernel<8>"),
    "packed": ("1", "0", "ldpc_layered_kernel<8, packed>"),
    "solo": ("0", "1", "ldpc_layered_kernel<8, solo>"),
    "packed-solo": ("1", "1", "ldpc_layered_kernel<8, packed, solo>"),
}
INPUTS = ["saturating", "near_threshold", "never_converging"]


def make(table, kind):
    N = T.ldpc_info(table)[0]
    if kind == "saturating":
        return T.make_input(table, "sat", G, seed=5)
    if kind == "never_converging":
        return T.llr_noise(G, N, seed=6)
    # codewords at amplitude 6; sigma from 3 (converges in a few updates at every rate here) to 9 (does not converge) over the batch
    clean, _ = T.llr_codeword_awgn(table, G, 7, amp=6.0, sigma=0.0)
    rng = np.random.default_rng(8)
    sigma = np.linspace(3.0, 9.0, G)[:, None]
    return np.clip(np.rint(clean.astype(np.float64) + sigma * rng.normal(0.0, 1.0, clean.shape)), -128, 127).astype(np.int8)


_want = {}


def expected(table, kind):
    if (table, kind) not in _want:
        llr = make(table, kind)
        if T.ref_ldpc() is not None:
            want, wret = T.ref_ldpc_decode(table, llr, 0, TRIALS)  # the genuine reference, AVX2 batch of 32 frames
        else:
            want, wret = T.oracle_ldpc_decode(table, llr, G, TRIALS)
        _want[(table, kind)] = (llr, want, wret)
    return _want[(table, kind)]


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("table", TABLES)
def test_class8_build_vs_reference(table, build, kind, monkeypatch):
    v2, solo, kernel = BUILDS[build]
    for k, v in {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": v2, "DVBS2_SOLO": solo}.items():
        monkeypatch.setenv(k, v)
    N, K, _, _ = T.ldpc_info(table)
    llr, want, wret = expected(table, kind)
    dec = LdpcDecoder(table=table, message_bits=K, group_size=G, max_frames=G, max_trials=TRIALS, outputmode=capi.OM_CODEWORD)
    assert dec.kernel_name == kernel
    bits, out, ret = dec.work(llr, want_llr=True)
    dec.close()
    assert ret.tolist() == wret, (table, build, kind)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"{table} {build} {kind}: LLR mismatch in frames {bad[:8]}"
    assert np.array_equal(bits, T.pack_bits(want, N))
