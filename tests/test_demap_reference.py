"""The soft demapper's CPU restatement (oracle/demap_oracle.c) against a float64 evaluation of the reference's formulas
(fec_testlib.demap_f64 / snr_f64): LLRs over a wide range of N0 and all three 8PSK column orders, exact ties and saturation
points built in float32, the SNR estimates, and the 8PSK column-order rule by rate name. No GPU: the GPU tests
(test_demap_paths_gpu.py) hold the kernels to the same restatement and the same float64 reference."""
import json
import os

import numpy as np
import pytest

import fec_testlib as T

N0_SWEEP = np.logspace(-3, 3, 7)  # 1e-3 .. 1e3
REQUIRED_TIES = (126.5, 127.5, -127.5, -128.5, 0.5, -0.5, 1.5, -1.5)
# N0 values at which the float32 search reaches every required tie (the product grid of x * scalar does not hit every k + 0.5 for
# every scalar): small, moderate, large, and at both ends of the float range
TIE_N0 = {4: (0.005, 0.3, 1000.0, 3e-30, 3e30), 8: (0.001, 0.7, 50.0, 3e30)}


def wide_symbols(nf, ns, seed):
    """Gaussian symbols whose magnitudes span 1e-4 .. 10: every N0 of the sweep sees LLRs across the quantiser's range."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-4, 1, (nf, ns))
    return (scale * (rng.normal(size=(nf, ns)) + 1j * rng.normal(size=(nf, ns)))).astype(np.complex64)


@pytest.mark.parametrize("constellation,order", [(4, 0), (8, 0), (8, 1), (8, 2)])
def test_restatement_llrs_vs_float64(constellation, order):
    """About 2.7 million symbols over N0 = 1e-3 .. 1e3: the restatement quantises the float64 value except where float32 rounding
    may decide (near_tie_mask), and those places are few."""
    ns = 32400 if constellation == 4 else 21600
    total = near_total = 0
    for i, n0 in enumerate(N0_SWEEP):
        syms = wide_symbols(4, ns, 100 * constellation + 10 * order + i)
        n0f = np.float32(n0) * np.array([1.0, 0.5, 2.0, 1.37], np.float32)  # one N0 per frame
        got = T.oracle_demap(syms, n0f, constellation, order)
        near_total += T.check_demap_vs_f64(got, syms, n0f, constellation, order, f"N0 {n0:g}")
        total += got.size
    print(f"constellation {constellation} order {order}: {near_total} near-tie LLRs of {total}")
    assert near_total < total * 1e-3


@pytest.mark.parametrize("constellation", [4, 8])
def test_restatement_exact_ties_round_to_even(constellation):
    """Symbols whose float32 product is exactly k + 0.5 (searched in numpy float32, the kernels' operation order): the restatement
    rounds ties to even (rintf / nearbyintf; roundf or (int)(v + 0.5f) would not) and saturates at 127 / -128."""
    for n0 in TIE_N0[constellation]:
        ties = T.tie_symbols(n0, constellation)
        assert set(REQUIRED_TIES) <= set(ties), (n0, sorted(set(REQUIRED_TIES) - set(ties)))
        assert len(ties) >= 150, (n0, len(ties))
        syms = np.array(list(ties.values()), np.complex64)[None, :]
        got = T.oracle_demap(syms, np.float32(n0), constellation, 0)
        pre = T.demap_f32_pre(syms[0], n0, constellation)
        if constellation == 4:
            got_n, pre_n = got[0].reshape(-1, 2).T, pre.reshape(-1, 2).T  # (re, im) rows
        else:
            ns = syms.shape[1]
            got_n = np.stack([got[0, :ns], got[0, ns:2 * ns], got[0, 2 * ns:]])  # order 0: b0, b1, b2 columns
            pre_n = np.stack(pre)
        for j, t in enumerate(ties):
            hit = np.nonzero(pre_n[..., j] == np.float32(t))
            assert hit[0].size, (n0, t)
            even = int(np.clip(2 * np.round(t / 2), -128, 127))  # the even neighbour of k + 0.5, saturated
            assert int(got_n[..., j][hit][0]) == even, (n0, t, int(got_n[..., j][hit][0]))
        assert np.array_equal(got_n, T.quantise_f64(pre_n.astype(np.float64)))  # every output, tie or not


def test_tie_expectations_spelled_out():
    """The even neighbours the tie test asserts, written out at the points where rounding modes differ."""
    want = {0.5: 0, -0.5: 0, 1.5: 2, -1.5: -2, 2.5: 2, 126.5: 126, 127.5: 127, -127.5: -128, -128.5: -128}
    assert {t: int(T.quantise_f64(np.array([t]))[0]) for t in want} == want


@pytest.mark.parametrize("constellation,order", [(4, 0), (8, 0), (8, 1), (8, 2)])
def test_restatement_edges_vs_float64(constellation, order):
    """Ties, far beyond saturation, +-0, zero, subnormals and (QPSK) +-inf at very small, moderate and very large N0."""
    for n0 in (1e-30, 1e-3, 0.7, 1e3, 1e30):
        s = T.edge_symbols(n0, constellation)
        ns = (s.size + 3) // 4 * 4
        syms = np.zeros((1, ns), np.complex64)
        syms[0, :s.size] = s
        got = T.oracle_demap(syms, np.float32(n0), constellation, order)
        T.check_demap_vs_f64(got, syms, np.float32(n0), constellation, order, f"N0 {n0:g}")
        if constellation == 4:
            inf_at = np.nonzero(np.isinf(s.view(np.float32)))[0]
            assert got[0, inf_at].tolist() == [127 if v > 0 else -128 for v in s.view(np.float32)[inf_at]]


def snr_rtol_sequential(n):
    """Sequential float32 sums of n positive terms (each term |x - s|^2 carries <= 4 u): <= (n + 3) u on each of the two sums,
    one more u for the quotient."""
    return (2 * (n + 3) + 1) * T.U32


@pytest.mark.parametrize("constellation,order", [(4, 0), (8, 0), (8, 1), (8, 2)])
def test_restatement_snr_vs_float64(constellation, order):
    """oracle_demap_snr (hard slice) and oracle_demap_snr_refined (signs of LLRs incl. 0 and -128) against snr_f64 within the
    restatement's own worst-case bound; noiseless frames hit the 1e-12 floor, all-zero frames give ~1."""
    ns = 32400 if constellation == 4 else 21600
    rng = np.random.default_rng(7 + order)
    idx = rng.integers(0, 8, (6, ns))
    pts = (np.exp(1j * (idx * np.pi / 4 + np.pi / 4)) if constellation == 4 else T.M8PSK[idx]).astype(np.complex64)
    if constellation == 4:  # the float constants of the QPSK points
        pts = (np.where(pts.real >= 0, T.RS2_F32, -T.RS2_F32) + 1j * np.where(pts.imag >= 0, T.RS2_F32, -T.RS2_F32)).astype(np.complex64)
    sigma = np.array([0.02, 0.1, 0.3, 1.0, 0, 0])[:, None]
    syms = (pts + sigma * (rng.normal(size=pts.shape) + 1j * rng.normal(size=pts.shape))).astype(np.complex64)
    syms[5] = 0
    rtol = snr_rtol_sequential(ns)
    got, want = T.oracle_snr(syms, constellation), T.snr_f64(syms, constellation)
    assert np.allclose(got, want, rtol=rtol, atol=0), (got, want, rtol)
    assert want[4] > 1e15 and abs(want[5] - 1) < 1e-6  # floor, and zero symbols against unit points
    llr = rng.integers(-128, 128, (6, ns * (2 if constellation == 4 else 3))).astype(np.int8)
    llr[:, :97] = 0
    llr[:, 97:200] = -128
    got, want = T.oracle_snr(syms, constellation, llr, order), T.snr_f64(syms, constellation, llr, order)
    assert np.allclose(got, want, rtol=rtol, atol=0), (got, want, rtol)


def test_column_order_rule_by_rate_name():
    """The reference's rule is written by rate name (lib/xfecframe_demapper_cb_impl.cc:50-69); the library decides by enumerator
    (demap_hip.hip: 4 -> "210"; 26, 28, 38, 39, 19 -> "102"). Through the enum values of dvb_config.h both say the same for every
    rate, and the GPU test checks Demapper.column_order against the same rule for every normal / short rate."""
    enums = json.load(open(os.path.join(T.ROOT, "tests", "golden", "dvb_config_enums.json")))["enums"]["dvb_code_rate_t"]
    library = {4: 1, 26: 2, 28: 2, 38: 2, 39: 2, 19: 2}
    for name, rid in enums.items():
        assert T.column_order(name) == library.get(rid, 0), name
    assert {n for n in enums if T.column_order(n)} == set(T.COLUMN_ORDER_210 + T.COLUMN_ORDER_102)
