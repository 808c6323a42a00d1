"""The encoder's host-only surface (dvbs2_enc_check, create without a device): needs no GPU. The answers to a null handle are
in tests/test_capi_null_handle.py.

dvbs2_enc_check is the verdict dvbs2_enc_create gives before it touches a device: DVBS2_OK exactly for the rows of
tests/golden/fec_params.json whose bch_n is the K of their LDPC table with n and k multiples of 8, combined with DVBS2_ENC_NO_MAPPER or a
constellation the row can carry; DVBS2_EINVAL with a text that names the argument otherwise."""
import ctypes as C
import json
import os

import fec_testlib as T
from dvbs2rx_amd import capi, ldpc_table_info

ROWS = json.load(open(os.path.join(T.ROOT, "tests", "golden", "fec_params.json")))["rows"]
APSK16 = ("C2_3", "C3_4", "C4_5", "C5_6", "C8_9", "C9_10")  # EN 302 307-1 table 12
APSK32 = ("C3_4", "C4_5", "C5_6", "C8_9", "C9_10")
CONSTELLATIONS = (capi.ENC_NO_MAPPER, capi.MOD_QPSK, capi.MOD_8PSK, capi.MOD_16APSK, capi.MOD_32APSK)


def _row_verdict(r):
    """None when the codes of the row can be encoded, else the beginning of the documented text."""
    if r["bch_n"] != ldpc_table_info(r["table"])["K"]:
        return b"rate: bch_n %d != table K %d of %s" % (r["bch_n"], ldpc_table_info(r["table"])["K"], r["table"].encode())
    if r["bch_n"] % 8 or r["bch_k"] % 8:
        return b"framesize: u8 array messages are only supported for n and k multiple of 8."
    return None


def _constellation_verdict(r, c):
    if c == capi.ENC_NO_MAPPER:
        return None
    if r["standard_id"] != capi.STANDARD_DVBS2:
        return b"constellation: a DVB-T2 rate has no built-in mapper"
    if c in (capi.MOD_QPSK, capi.MOD_8PSK):
        return None  # as the demapper: every DVB-S2 / S2X rate
    if r["framesize_id"] == capi.FECFRAME_MEDIUM:
        return b"framesize: Unsupported frame size for 16APSK / 32APSK"
    ok = r["rate"] in (APSK16 if c == capi.MOD_16APSK else APSK32) and not (r["rate"] == "C9_10" and r["framesize_id"] != capi.FECFRAME_NORMAL)
    return None if ok else b"constellation: Unsupported code rate for 16APSK / 32APSK"


def test_check_verdict_for_every_row_and_constellation():
    n_ok = n_shortened = 0
    for r in ROWS:
        for c in CONSTELLATIONS:
            want = _row_verdict(r) or _constellation_verdict(r, c)
            rc = capi.lib.dvbs2_enc_check(r["standard_id"], r["framesize_id"], r["rate_id"], c)
            what = (r["standard"], r["framesize"], r["rate"], c)
            if want is None:
                assert rc == capi.OK, (what, capi.lib.dvbs2_last_error())
                n_ok += 1
            else:
                assert rc == capi.EINVAL and capi.lib.dvbs2_last_error().startswith(want), (what, rc, capi.lib.dvbs2_last_error(), want)
                n_shortened += want.startswith(b"rate: bch_n")
    assert n_ok > 100 and n_shortened >= len(CONSTELLATIONS)  # both kinds of row exist in the fixture


def test_check_refuses_what_no_row_has():
    assert capi.lib.dvbs2_enc_check(0, 1, 999, capi.ENC_NO_MAPPER) == capi.EINVAL
    assert capi.lib.dvbs2_last_error() == b"unsupported (standard, framesize, rate)"
    for c in (1, 2, -2, -3, 12):
        assert capi.lib.dvbs2_enc_check(0, 1, 3, c) == capi.EINVAL
        assert capi.lib.dvbs2_last_error().startswith(b"constellation: Unsupported constellation")


def test_the_shortened_rows_are_refused_by_name():
    bad = [r for r in ROWS if r["bch_n"] != ldpc_table_info(r["table"])["K"]]
    assert bad
    for r in bad:
        assert capi.lib.dvbs2_enc_check(r["standard_id"], r["framesize_id"], r["rate_id"], capi.ENC_NO_MAPPER) == capi.EINVAL
        text = capi.lib.dvbs2_last_error()
        assert r["table"].encode() in text and b"dvbs2_enc_create_parts encodes the mother code" in text, text


def test_create_judges_its_arguments_before_the_device():
    h = C.c_void_p(1)
    assert capi.lib.dvbs2_enc_create(C.byref(h), 0, 1, 3, capi.MOD_32APSK, 4, 0) == capi.EINVAL and not h
    assert capi.lib.dvbs2_last_error().startswith(b"constellation: Unsupported code rate")
    pts = (C.c_float * 512)(*([0.5] * 512))
    h = C.c_void_p(1)
    assert capi.lib.dvbs2_enc_create_table(C.byref(h), 0, 1, 3, 7, pts, None, 4, 0) == capi.EINVAL and not h
    assert capi.lib.dvbs2_last_error().startswith(b"n_mod 7 is not supported")
    col = (C.c_uint8 * 8)(0, 1, 2, 2, 4, 5, 6, 7)
    assert capi.lib.dvbs2_enc_create_table(C.byref(h), 0, 1, 3, 6, pts, col, 4, 0) == capi.EINVAL
    assert capi.lib.dvbs2_last_error().startswith(b"column is not a permutation")
    assert capi.lib.dvbs2_enc_create_table(C.byref(h), 0, 1, 3, 6, None, None, 4, 0) == capi.EINVAL
    assert capi.lib.dvbs2_last_error() == b"points_re_im is NULL"
    assert capi.lib.dvbs2_enc_create_parts(C.byref(h), 0, 0, 0, 0, None, 4, 0) == capi.EINVAL
    assert capi.lib.dvbs2_last_error() == b"at least one of the BCH and the LDPC stage is required"
    assert capi.lib.dvbs2_enc_create_parts(C.byref(h), 0, 0, 0, 0, b"S2_TABLE_NONE", 4, 0) == capi.EINVAL
    assert capi.lib.dvbs2_last_error() == b"ldpc_table: unknown LDPC table S2_TABLE_NONE"
    assert capi.lib.dvbs2_enc_create(None, 0, 1, 3, capi.MOD_QPSK, 4, 0) == capi.EINVAL
    assert capi.lib.dvbs2_last_error() == b"null handle pointer"


def test_create_without_a_device_is_edevice():
    h = C.c_void_p()
    if capi.lib.dvbs2_device_count() == 0:
        assert capi.lib.dvbs2_enc_create(C.byref(h), 0, 1, 3, capi.MOD_QPSK, 4, 0) == capi.EDEVICE and not h
        assert b"no HIP device" in capi.lib.dvbs2_last_error()
        assert capi.lib.dvbs2_enc_create_parts(C.byref(h), 0, 0, 0, 0, b"S2_TABLE_C1", 4, 0) == capi.EDEVICE and not h
    else:  # with one: a device index it does not have
        assert capi.lib.dvbs2_enc_create(C.byref(h), 0, 1, 3, capi.MOD_QPSK, 4, 99) == capi.EINVAL and not h
        assert capi.lib.dvbs2_last_error() == b"device index out of range"
