"""Edge cases of the packed check node (check_node_v2 and its chain / hazard siblings) in the degree classes 8 and 16: whole frames of
crafted LLRs through the packed builds, bit-exact against the genuine reference decoder in oracle/_ref (the plain-C restatement where
that was not built) on decoded LLRs, packed bits and per-group return values.

The inputs aim at the spots where the packed arithmetic differs from the reference's int8 code: saturated halves (0x7fff magnitudes,
the -128 input), ties at the minimum (the selection of the "other" magnitude), zero inputs (sign of zero, R2's floor) and magnitudes
around 31 / 32, where the stored message's asymmetric clamp (R7, -32 .. 31) switches."""
import zlib

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import LdpcDecoder, capi

pytestmark = pytest.mark.gpu

BUILDS = {  # (table, forced build) -> the kernel the handle must launch
    "B4-packed-solo": ("S2_TABLE_B4", {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "1"},
                       "ldpc_layered_kernel<8, packed, solo>"),
    "B4-packed-pair": ("S2_TABLE_B4", {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "0"},
                       "ldpc_layered_kernel<8, packed>"),
    "B7-packed-solo": ("S2_TABLE_B7", {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "1"},
                       "ldpc_layered_kernel<16, packed, solo>"),
    "B7-packed-pair": ("S2_TABLE_B7", {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "0"},
                       "ldpc_layered_kernel<16, packed>"),
}
G = 32


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1, 1)


def _codeword_signs(table, n, seed):
    """+1 / -1 per bit of random codewords (bit 0 -> positive LLR, the reference's convention)."""
    llr, _ = T.llr_codeword_awgn(table, n, seed, amp=20.0, sigma=0.0)
    return np.where(llr.astype(np.int32) < 0, -1, 1)


def inputs(table, case):
    N = T.ldpc_info(table)[0]
    rng = np.random.default_rng(zlib.crc32(f"{table}:{case}".encode()))
    if case == "saturated":  # every LLR at +127, -127 or -128
        return rng.choice(np.array([127, -127, -128], np.int8), (G, N))
    if case == "saturated_codewords":  # saturated magnitudes on codeword signs, a fifth of them flipped: the frames converge
        s = _codeword_signs(table, G, 11)
        s = np.where(rng.random(s.shape) < 0.2, -s, s)
        return np.where(s < 0, rng.choice(np.array([-127, -128]), s.shape), 127).astype(np.int8)
    if case == "ties":  # one magnitude everywhere: every check is tied at its minimum in the first update
        return (_signs(rng, (G, N)) * 9).astype(np.int8)
    if case == "near_ties":  # two levels, so that minimum and second minimum are often equal
        return (_signs(rng, (G, N)) * rng.choice(np.array([4, 4, 4, 5]), (G, N))).astype(np.int8)
    if case == "zeros":
        return np.zeros((G, N), np.int8)
    if case == "zeros_mixed":  # zeros among small values of both signs (sign of a zero input, R2's floor at 0 and 1)
        return rng.choice(np.array([0, 0, 1, -1, 2, -2], np.int8), (G, N))
    if case == "clamp_31_32":  # magnitudes around the stored message's clamp (R7: -32 .. 31)
        return (_signs(rng, (G, N)) * rng.choice(np.array([30, 31, 32, 33, 34]), (G, N))).astype(np.int8)
    if case == "clamp_codewords":  # the same on codeword signs with flips: many updates with messages at the clamp
        s = _codeword_signs(table, G, 12)
        s = np.where(rng.random(s.shape) < 0.15, -s, s)
        return (s * rng.choice(np.array([31, 32, 33]), s.shape)).astype(np.int8)
    raise KeyError(case)


CASES = ["saturated", "saturated_codewords", "ties", "near_ties", "zeros", "zeros_mixed", "clamp_31_32", "clamp_codewords"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("build", list(BUILDS))
def test_packed_node_edges(build, case, monkeypatch):
    table, env, kernel = BUILDS[build]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N, K, _, _ = T.ldpc_info(table)
    llr = inputs(table, case)
    trials = 12
    dec = LdpcDecoder(table=table, message_bits=K, group_size=G, max_frames=G, max_trials=trials, outputmode=capi.OM_CODEWORD)
    assert dec.kernel_name == kernel
    bits, out, ret = dec.work(llr, want_llr=True)
    dec.close()
    if T.ref_ldpc() is not None:
        want, wret = T.ref_ldpc_decode(table, llr, 0, trials)  # the genuine reference, AVX2 batch of 32 frames
    else:
        want, wret = T.oracle_ldpc_decode(table, llr, G, trials)
    assert ret.tolist() == wret, (build, case)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"{build} {case}: LLR mismatch in frames {bad[:8]}"
    assert np.array_equal(bits, T.pack_bits(want, N))
