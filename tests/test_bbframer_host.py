"""CPU: the host-only code of the BB framer -- BBHEADER, CRC-8, the packet arithmetic of a call and the argument checks -- once more in a
stand-alone program built with the host sanitizers, over good and refused arguments. Its answers must be those of the restatements in
fec_testlib, of the reference's known CRC answers, of the model's need() and of the library's own entries."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fec_testlib as T
from bbframer_model import BbFramerModel
from dvbs2rx_amd import bbheader_build, capi, crc8

HDR_TEXT = "matype1, matype2 and sync must be in 0..255, upl_bits, dfl_bits and syncd_bits in 0..65535"


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/bbframer_host_main.cpp with the source it calls, host code under AddressSanitizer and UBSan (device code is not instrumented
    and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("bbframer"), "bbframer_host_main.cpp", ("bbframer_hip.hip",))


def _lib_refuses_create(kbch_bits, max_frames):
    h = C.c_void_p()
    rc = capi.lib.dvbs2_bbframer_create_raw(C.byref(h), kbch_bits, max_frames, 0)
    assert rc == capi.EINVAL and not h  # every row below is refused before a device is looked for
    return capi.lib.dvbs2_last_error().decode()


def _lib_header(args):
    h = np.zeros(10, np.uint8)
    rc = capi.lib.dvbs2_bbheader_build(h.ctypes.data, *args)
    return rc, h


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(31)
    rows, want = [], []
    # BBHEADER: the fields at both ends, every SYNCD a framer can write, random ones
    hdrs = [(0xF2, 0, 1504, 58112, 0x47, 0), (0xF1, 0x2A, 1504, 1504, 0x47, 1496), (0, 0, 0, 0, 0, 0), (255, 255, 65535, 65535, 255, 65535)]
    hdrs += [(0xF2, 0, 1504, 15928, 0x47, 8 * s) for s in range(188)]
    hdrs += [tuple(int(v) for v in (rng.integers(0, 256), rng.integers(0, 256), rng.integers(0, 65536), rng.integers(0, 65536),
                                    rng.integers(0, 256), rng.integers(0, 65536))) for _ in range(20)]
    for a in hdrs:
        rows.append("hdr %d %d %d %d %d %d" % a)
        m1, m2, upl, dfl, sync, syncd = a
        w = T.bbheader(0, syncd, dfl, upl, m1, m2, sync)
        want.append(bytes(w).hex())
        rc, h = _lib_header(a)
        assert rc == capi.OK and np.array_equal(h, w) and np.array_equal(bbheader_build(*a), w)
    bad_hdrs = [(256, 0, 1504, 8, 0x47, 0), (-1, 0, 1504, 8, 0x47, 0), (0, 256, 1504, 8, 0x47, 0), (0, 0, 65536, 8, 0x47, 0),
                (0, 0, 1504, 65536, 0x47, 0), (0, 0, 1504, -8, 0x47, 0), (0, 0, 1504, 8, 256, 0), (0, 0, 1504, 8, 0x47, 65536),
                (0, 0, 1504, 8, 0x47, -1)]
    for a in bad_hdrs:
        rows.append("hdr %d %d %d %d %d %d" % a)
        want.append("refused")
        rc, _ = _lib_header(a)
        assert rc == capi.EINVAL and capi.lib.dvbs2_last_error().decode() == HDR_TEXT
    # CRC-8: nothing, one byte, a packet, long strings; the reference's known remainders (rem(d) = check(d[:-1]) ^ d[-1])
    strings = [b"", b"\x00", b"\x01", b"\xff"] + [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (2, 9, 187, 188, 1000)]
    for d in strings:
        rows.append("crc %d %s" % (len(d), d.hex() or "-"))
        want.append(str(T.crc8_dvbs2(d)))
        assert crc8(d) == T.crc8_dvbs2(d)
    gold = json.load(open(os.path.join(T.ROOT, "tests", "golden", "crc8_golden.json")))["cases"]
    assert len(gold) >= 20
    for c in gold:
        d = bytes.fromhex(c["hex"])
        rows.append("crc %d %s" % (len(d) - 1, d[:-1].hex() or "-"))
        want.append(str(c["rem"] ^ d[-1]))
        assert crc8(d[:-1]) == c["rem"] ^ d[-1]
    # need: pos at every residue mod 188 (and far into a stream), against the model
    m = BbFramerModel(16008)
    n_need = 0
    for r in range(188):
        for base in (0, 188 * 1000, 188 * (1 << 40)):
            for n, dfl in ((0, 188), (1, 188), (1, 189), (3, 1991), (7, 1880), (65535, 8191)):
                m.pos = base + r
                rows.append(f"need {base + r} {n} {dfl}")
                m.max_dfl_bytes = max(m.max_dfl_bytes, dfl)
                want.append(str(m.need(n, dfl)))
                n_need += 1
    # create: the corners of kbch_bits and max_frames
    for kbch, mf in ((1584, 1), (65608, 65535), (3072, 64), (58192, 4096)):
        rows.append(f"create {kbch} {mf}")
        want.append("ok")
    bad_creates = ((1576, 1), (65616, 1), (65624, 1), (80, 1), (3073, 1), (-8, 1), (3072, 0), (3072, 65536), (3072, -1))
    for kbch, mf in bad_creates:
        rows.append(f"create {kbch} {mf}")
        want.append("refused: " + _lib_refuses_create(kbch, mf))
    assert _lib_refuses_create(1576, 1).startswith("kbch_bits") and _lib_refuses_create(3072, 0).startswith("max_frames")
    # a call: dfl_bytes and n_frames at their ends
    mx = 3072 // 8 - 10
    for n, dfl in ((0, 0), (1, 0), (64, 188), (64, mx), (0, mx)):
        rows.append(f"call 64 {mx} {n} {dfl}")
        want.append("ok")
    for n, dfl, w in ((1, 187, "refused -1: dfl_bytes must be 0 or in 188..max_dfl_bytes"), (1, mx + 1, "refused -1: dfl_bytes must be 0 or in 188..max_dfl_bytes"),
                      (1, -1, "refused -1: dfl_bytes must be 0 or in 188..max_dfl_bytes"), (65, 0, "refused -3: n_frames must be in 0..max_frames"),
                      (-1, 0, "refused -3: n_frames must be in 0..max_frames")):
        rows.append(f"call 64 {mx} {n} {dfl}")
        want.append(w)
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows)
    for row, got, w in zip(rows, lines, want):
        assert got == w, row[:60]
    assert sum(w.startswith("refused") for w in want) == len(bad_hdrs) + len(bad_creates) + 5 and n_need == 188 * 3 * 6


def test_host_entries_answer_null():
    assert capi.lib.dvbs2_bbheader_build(None, 0, 0, 0, 0, 0, 0) == capi.EINVAL and capi.lib.dvbs2_last_error() == b"out is null"
    assert capi.lib.dvbs2_crc8(None, 3) == capi.EINVAL and capi.lib.dvbs2_last_error() == b"data is null"
    assert capi.lib.dvbs2_crc8(None, 0) == 0
