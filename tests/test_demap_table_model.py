"""The caller-table demapper without a device: the verdicts and texts of dvbs2_demap_table_check (host only), the inputs of the GPU
demapper test under the float64 rule with the float32 model alone, and the two end-to-end operating points through the model
demapper and the CPU LDPC decoder. The tables are test material (tests/demap_table_model.py), not any standard's."""
import ctypes as C

import numpy as np
import pytest

import apsk_model as A
import demap_table_model as D
import fec_testlib as T
from dvbs2rx_amd import capi, demap_table_check


def _check(n_mod, pts, column):
    """(return code, text) of dvbs2_demap_table_check on raw arguments"""
    p = None if pts is None else np.ascontiguousarray(pts, np.complex64)
    c = None if column is None else np.ascontiguousarray(column, np.uint8)
    rc = capi.lib.dvbs2_demap_table_check(n_mod, p.ctypes.data if p is not None else None, c.ctypes.data if c is not None else None)
    return rc, capi.lib.dvbs2_last_error().decode()


def test_table_check_verdicts():
    rng = np.random.default_rng(1)
    for p in (D.FOUR, D.RING8, D.RING64, D.RING256, D.gray_qam(6), D.gray_qam(8), A.points(A.MOD_16APSK, "C2_3"), A.points(A.MOD_32APSK, "C3_4")):
        n_mod = int(np.log2(len(p)))
        assert _check(n_mod, p, None)[0] == capi.OK
        assert _check(n_mod, p, D.natural(n_mod))[0] == capi.OK
        assert _check(n_mod, p, rng.permutation(n_mod))[0] == capi.OK
        assert _check(n_mod, 1e3 * p, n_mod - 1 - np.arange(n_mod))[0] == capi.OK  # not scaled, Es = 1 not required
        demap_table_check(p, rng.permutation(n_mod))
    big = np.zeros(512, np.complex64)
    for n_mod, text in ((1, "n_mod"), (9, "n_mod"), (0, "n_mod"), (-1, "n_mod"), (7, "n_mod 7")):
        rc, why = _check(n_mod, big, None)
        assert rc == capi.EINVAL and text in why, (n_mod, why)
    assert "multiple of 7" in _check(7, big, None)[1]  # a message of its own
    rc, why = _check(6, None, None)
    assert rc == capi.EINVAL and "points_re_im" in why
    for bad in (np.nan, np.inf, -np.inf):
        for part in (0, 1):
            p = D.RING64.astype(np.complex64)
            v = p.view(np.float32)
            v[2 * 37 + part] = bad
            rc, why = _check(6, p, None)
            assert rc == capi.EINVAL and "points_re_im" in why and "37" in why, why
    for column in ((0, 1, 2, 3, 4, 4), (0, 0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 6), (255, 1, 2, 3, 4, 5)):
        rc, why = _check(6, D.RING64, column)
        assert rc == capi.EINVAL and "column" in why, why
    with pytest.raises(capi.Dvbs2Error, match="column"):
        demap_table_check(D.RING8, (0, 1, 1))
    # create gives the verdict of the check before it looks for a device, and leaves the handle null
    h = C.c_void_p(1)
    p = D.RING64.astype(np.complex64)
    assert capi.lib.dvbs2_demap_create_table(C.byref(h), D.SHORT, 7, p.ctypes.data, None, 4, 0) == capi.EINVAL and not h.value
    assert "multiple of 7" in capi.lib.dvbs2_last_error().decode()
    h = C.c_void_p(1)
    assert capi.lib.dvbs2_chain_create_table(C.byref(h), capi.STANDARD_DVBS2, D.SHORT, 6, 6, None, None, 8, 8, 0) == capi.EINVAL and not h.value
    assert "points_re_im" in capi.lib.dvbs2_last_error().decode()


def test_test_tables():
    for p in D.TABLES.values():
        assert abs(np.mean(np.abs(p) ** 2) - 1.0) < 1e-12
        assert len({(round(z.real, 9), round(z.imag, 9)) for z in p}) == len(p)
    assert np.sum(np.abs(D.RING8) < 1e-12) == 1  # the point at the origin
    for n_mod in (6, 8):
        p, h = D.gray_qam(n_mod), n_mod // 2
        assert abs(np.mean(np.abs(p) ** 2) - 1.0) < 1e-12
        step = np.min(np.abs(p[:, None] - p[None, :])[~np.eye(len(p), dtype=bool)])
        for i, z in enumerate(p):  # Gray: nearest neighbours differ in one label bit
            for k, w in enumerate(p):
                if abs(abs(z - w) - step) < 1e-9:
                    assert bin(i ^ k).count("1") == 1
        assert np.allclose(p[5 << h].real, p[(5 << h) | 3].real)  # the upper bits select the real axis


def test_columns_round_trip():
    rng = np.random.default_rng(2)
    for p, column in ((D.RING64, (2, 1, 0, 5, 3, 4)), (D.RING256, (7, 0, 6, 1, 5, 2, 4, 3)), (D.RING8, (0, 1, 2))):
        n_mod = len(column)
        bits = rng.integers(0, 2, (2, n_mod * 40), dtype=np.uint8)
        syms = D.map_bits_columns(bits, p, column).astype(np.complex64)
        nat = A.demap_f32(syms, 1e-4, p.astype(np.complex64))[0]  # small enough that no LLR of these tables rounds to 0
        llr = D.permute_columns(nat, n_mod, column)
        assert np.array_equal((llr < 0).astype(np.uint8), bits)  # noiseless hard decisions give the bits back through column[]
        assert np.array_equal(D.unpermute_columns(llr, n_mod, column), nat)
        assert np.array_equal(D.map_bits_columns(bits, p, D.natural(n_mod)), A.map_bits(bits, p))


@pytest.mark.parametrize("name,table,framesize,column", D.CASES, ids=[c[0] for c in D.CASES])
def test_gpu_inputs_meet_the_float64_rule(name, table, framesize, column):
    """The float32 model on the inputs of test_demap_table_gpu.py: a difference from float64 is one step, lies within delta of a
    half-integer, and the share is at most 4 delta (apsk_model.check_vs_f64) -- a condition these inputs meet, not a tolerance.
    Measured on these inputs: 0 differing LLRs in every case but the 256-point table on medium frames (4 of 96 960, each within
    8e-6 of a half-integer), against caps of several hundred to several thousand (printed)."""
    syms, per_frame, one, p, _, one_n0 = D.demap_case(table, framesize)
    n_mod = int(np.log2(len(p)))
    rows = syms.shape[1]
    keep, sel = D.unplanted(rows, n_mod)
    for want, n0 in ((per_frame, D.N0_FRAMES), (one, one_n0)):
        n_diff, delta, _ = A.check_vs_f64(want[:, sel], syms[:, keep], n0, p, name + " model")
        print(f"{name}: cap {4.0 * delta * want[:, sel].size:.1f}, distinct LLR values per frame {[len(np.unique(w)) for w in want]}, "
              f"saturated share per frame {[round(float(np.mean((w == 127) | (w == -128))), 3) for w in want]}")
    if len(p) == 256:
        assert all(len(np.unique(w)) > 32 for w in per_frame[1:])  # magnitudes are exercised (6 or 7 distinct values at N0 0.2)
    if name == D.SATURATION_CASE:
        sat = np.mean((one[0] == 127) | (one[0] == -128))
        print(f"{name}: saturated share of frame 0 at N0 {one_n0} {sat:.3f}")
        assert 0.05 < sat < 0.25


@pytest.mark.parametrize("name", list(D.E2E))
def test_end_to_end_operating_point(name):
    """Gray 64-QAM, column [2, 1, 0, 5, 3, 4], at Es/N0 17.5 dB and Gray 256-QAM, column [7, 0, 6, 1, 5, 2, 4, 3], at 22.5 dB: 8 short
    3/4 frames (S2_TABLE_C7), G = 8, 50 trials, model demapper -> CPU LDPC decoder. The rule: the smallest 0.5 dB step at which
    all 8 frames decode, plus 1.5 dB. Found with the seeds of demap_table_model.e2e_case: 16.0 dB and 21.0 dB (no frame decodes
    half a dB below either), hard-decision bit error rates before the decoder there 0.052 and 0.054; at the operating points
    0.031 and 0.036."""
    n_mod, column, es_n0_db = D.E2E[name]
    sent, cw, syms, n0, p = D.e2e_case(name)
    llr = D.permute_columns(A.demap_f32(syms, n0, p.astype(np.complex64))[0], n_mod, column)
    ber = np.mean((llr < 0).astype(np.uint8) != cw)
    out, rets = T.cpu_ldpc_decode_ragged(D.E2E_TABLE, llr, D.E2E_GROUP, D.E2E_TRIALS)
    print(f"{name} at {es_n0_db} dB: hard-decision bit error rate before the decoder {ber:.4f}, LDPC ret {rets}")
    assert all(r >= 0 for r in rets)
    assert np.array_equal((out < 0).astype(np.uint8), cw)  # every frame decodes
    assert 1e-3 < ber < 0.1  # the decoder had work to do
