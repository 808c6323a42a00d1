"""16APSK / 32APSK without a device: the library's constellation table (dvbs2_apsk_points, host only) against the table typed in
from EN 302 307-1 in tests/apsk_model.py, the internal consistency of that table, and the float32 restatement of the kernel's
arithmetic against the float64 max-log model. The tables are UNPINNED (see apsk_model.py)."""
import json
import os

import numpy as np
import pytest

import apsk_model as A
import fec_testlib as T
from dvbs2rx_amd import apsk_points, capi
from dvbs2rx_amd.blocks import rate_id


def test_macros_match_the_reference_enums():
    with open(os.path.join(T.ROOT, "tests", "golden", "dvb_config_enums.json")) as f:
        groups = json.load(f)["enums"]
    enums = {**groups["dvb_constellation_t"], **groups["dvb_code_rate_t"]}
    assert enums["MOD_16APSK"] == capi.MOD_16APSK == A.MOD_16APSK == 6
    assert enums["MOD_32APSK"] == capi.MOD_32APSK == A.MOD_32APSK == 8
    with open(os.path.join(T.ROOT, "include", "dvbs2_fec_hip.h")) as f:
        hdr = f.read()
    assert "#define DVBS2_MOD_16APSK 6\n" in hdr and "#define DVBS2_MOD_32APSK 8\n" in hdr
    for name in list(A.GAMMA_16) + list(A.GAMMA_32):
        assert rate_id(name) == enums[name]


@pytest.mark.parametrize("constellation,rate", A.PAIRS)
def test_library_table_equals_the_model(constellation, rate):
    got = apsk_points(constellation, rate)
    want = A.points(constellation, rate)
    assert got.dtype == np.complex64 and got.shape == want.shape == (1 << A.N_MOD[constellation],)
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        w32 = w.astype(np.float32)
        # one float ulp of the value (the model's own value rounded to float is the expected entry)
        assert (np.abs(g.astype(np.float64) - w32) <= np.spacing(np.abs(w32))).all()
        assert (np.abs(g.astype(np.float64) - w) <= 2.0 ** -23 * np.maximum(np.abs(w), 2.0 ** -126) + 1e-16).all()


@pytest.mark.parametrize("constellation,rate", A.PAIRS)
def test_table_consistency(constellation, rate):
    n_mod = A.N_MOD[constellation]
    p = A.points(constellation, rate)
    assert abs(np.mean(np.abs(p) ** 2) - 1.0) < 1e-15  # Es = 1
    assert len({(round(z.real, 12), round(z.imag, 12)) for z in p}) == len(p) == 1 << n_mod  # every label its own point
    rad = A.radii(constellation, rate)
    assert all(a < b for a, b in zip(rad, rad[1:]))
    sizes = [len(A.ring_walk(constellation, r)) for r in range(len(rad))]
    assert sizes == ([4, 12] if constellation == A.MOD_16APSK else [4, 12, 16])
    # Gray along the 4- and the 12-point ring of either constellation and along nothing more: the 32APSK outer ring is only
    # quasi-Gray in the standard
    for ring in (0, 1):
        w = A.ring_walk(constellation, ring)
        ang = np.mod([A.ring_angle(constellation)[i][1] for i in w], 2 * np.pi)
        assert np.allclose(np.diff(ang), 2 * np.pi / len(w))  # equally spaced
        for a, b in zip(w, w[1:] + w[:1]):
            assert bin(a ^ b).count("1") == 1, (ring, a, b)
    if constellation == A.MOD_16APSK:  # the two low label bits are the signs of im and re (the mirror symmetry of the labels)
        for i, z in enumerate(p):
            assert (z.imag < 0) == bool(i & 1) and (z.real < 0) == bool(i & 2)
            assert np.isclose(p[i ^ 1], np.conj(z)) and np.isclose(p[i ^ 2], -np.conj(z))


def test_rejected_combinations():
    buf = np.empty(64, np.float32)
    lib = capi.lib
    ok16, ok32 = set(A.GAMMA_16), set(A.GAMMA_32)
    for r in range(0, 48):
        name = lib.dvbs2_rate_name(r)
        name = name.decode() if name else None
        assert lib.dvbs2_apsk_points(capi.MOD_16APSK, r, buf.ctypes.data) == (capi.OK if name in ok16 else capi.EINVAL), (r, name)
        assert lib.dvbs2_apsk_points(capi.MOD_32APSK, r, buf.ctypes.data) == (capi.OK if name in ok32 else capi.EINVAL), (r, name)
    assert lib.dvbs2_apsk_points(capi.MOD_16APSK, -1, buf.ctypes.data) == capi.EINVAL
    assert b"rate" in lib.dvbs2_last_error()
    for c in (capi.MOD_QPSK, 1, 2, 3, capi.MOD_8PSK, 5, 7, 9, -1):
        assert lib.dvbs2_apsk_points(c, rate_id("C3_4"), buf.ctypes.data) == capi.EINVAL
        assert b"Unsupported constellation" in lib.dvbs2_last_error()
    assert lib.dvbs2_apsk_points(capi.MOD_16APSK, rate_id("C3_4"), None) == capi.EINVAL


def test_mapper_and_layout_round_trip():
    """hard decisions on noiseless LLRs give the codeword bits back through the column layout"""
    rng = np.random.default_rng(3)
    for constellation, rate in ((A.MOD_16APSK, "C2_3"), (A.MOD_32APSK, "C3_4")):
        p = A.points(constellation, rate)
        n_mod = A.N_MOD[constellation]
        bits = rng.integers(0, 2, (2, n_mod * 50), dtype=np.uint8)
        syms = A.map_bits(bits, p).astype(np.complex64)
        for llr in (A.demap_f64(syms, 0.1, p), A.demap_f32(syms, 0.1, p.astype(np.complex64))[0]):
            assert np.array_equal((llr < 0).astype(np.uint8), bits)
        assert np.allclose(A.snr_f64(syms, p, A.demap_f64(syms, 0.1, p)), A.snr_f64(syms, p))


@pytest.mark.parametrize("constellation,rate", [(A.MOD_16APSK, "C2_3"), (A.MOD_16APSK, "C9_10"), (A.MOD_32APSK, "C3_4"), (A.MOD_32APSK, "C9_10")])
@pytest.mark.parametrize("n0", [0.2, 0.05, 0.01])
def test_restatement_against_float64(constellation, rate, n0):
    """200 000 symbols = point + complex Gaussian noise of variance N0. The float32 restatement (on the LIBRARY's float table) may
    differ from the float64 model (on the model's own table) by one step where the float64 value is within delta of a half-integer,
    delta = 16 * 2^-24 * D_max / N0 (apsk_model.delta_bound), and on no more than a share of 4 delta of the LLRs."""
    n = 200000
    rng = np.random.default_rng(1000 * constellation + int(n0 * 1000) + len(rate))
    p = A.points(constellation, rate)
    tx = p[rng.integers(0, len(p), n)]
    y = (tx + np.sqrt(n0 / 2.0) * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)[None, :]
    got, L32 = A.demap_f32(y, np.float32(n0), apsk_points(constellation, rate))
    L64, d_max = A.maxlog_f64(y, np.float32(n0), p)
    err = np.abs(L32.astype(np.float64) - L64).max()
    n_diff, delta, _ = A.check_vs_f64(got, y, np.float32(n0), p, f"{'16' if constellation == 6 else '32'}APSK {rate} N0 {n0}")
    print(f"largest |float32 - float64| before rounding {err:.3e}, saturated share {np.mean((got == 127) | (got == -128)):.3f}")
    assert err <= delta
    assert delta < 0.01  # the excuse covers a sliver of the LLRs, not the test
