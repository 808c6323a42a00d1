"""CPU: the host side of the de-header rows' C ABI -- rows_check, rows_geometry, state_counters and the argument checks of the device
entry, which refuses before a device is looked for -- through the library and in a stand-alone program built with the host sanitizers
(tests/bbdeheader_rows_host_main.cpp). The program's answers must be the library's own. Nothing is loaded into Python by the program
and no GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import BBDEHEADER_STATE, bbdeheader_rows_check, bbdeheader_rows_geometry, bbdeheader_state_counters, capi

SOURCES = ("c_api_bbdeheader_rows.hip", "bbdeheader_rows_hip.hip")  # the entries' translation unit and what it binds
lib = capi.lib


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return T.build_host_program(tmp_path_factory.mktemp("bbdeheader_rows"), "bbdeheader_rows_host_main.cpp", SOURCES)


def said(rc):
    return "ok" if rc == capi.OK else f"refused {rc}: {lib.dvbs2_last_error().decode()}"


KBCH_TEXT = "kbch_bits must be a multiple of 8 in 88..65615"
STREAMS_TEXT = "n_streams out of range (1..1024)"
FRAMES_TEXT = "max_frames out of range (1..2^20)"
# (kbch_bits, n_streams, max_frames) -> None or the refusal: the corners of every range
CHECKS = [((88, 1, 1), None), ((65615 - 7, 1024, 1 << 20), None), ((3072, 5, 700), None), ((16008, 1, 1), None), ((58192, 1024, 4096), None),
          ((80, 1, 1), KBCH_TEXT), ((87, 1, 1), KBCH_TEXT), ((3076, 1, 1), KBCH_TEXT), ((65616, 1, 1), KBCH_TEXT), ((0, 1, 1), KBCH_TEXT),
          ((-8, 1, 1), KBCH_TEXT), ((3072, 0, 1), STREAMS_TEXT), ((3072, 1025, 1), STREAMS_TEXT), ((3072, -1, 1), STREAMS_TEXT),
          ((3072, 1, 0), FRAMES_TEXT), ((3072, 1, (1 << 20) + 1), FRAMES_TEXT), ((3072, 1, -1), FRAMES_TEXT),
          ((80, 0, 0), KBCH_TEXT), ((3072, 0, 0), STREAMS_TEXT)]  # the first argument that is wrong is the one named

# addresses that are never dereferenced: 16-byte aligned ones, one at +8, one at +4, one at +2
A, B8, C4, D2 = 0x10000, 0x20008, 0x30004, 0x40002
ROWS_NAMES = ("d_bbframes", "kbch_bits", "d_offsets", "n_streams", "max_frames", "d_state", "d_work", "work_bytes", "d_ts_out", "out_bytes", "d_pkt_offsets")
POINTERS = (0, 2, 5, 6, 8, 10)


def good_rows(kbch=3072, S=5, mf=700):
    g = bbdeheader_rows_geometry(kbch, S, mf)
    return (A + 1, kbch, 0x50000, S, mf, 0x60000, 0x70000, g["work_bytes"], 0x80001, g["out_bytes"], 0x90004)


def with_(args, **changes):
    a = list(args)
    for k, v in changes.items():
        a[ROWS_NAMES.index(k)] = v
    return tuple(a)


def rows_refused():
    """(arguments, code, text) of every refusal of the device entry"""
    good = good_rows()
    g = bbdeheader_rows_geometry(3072, 5, 700)
    size = lambda name: f"{name} is below the geometry's {g[name]}"  # noqa: E731
    E, Z = capi.EINVAL, capi.ESIZE
    return [(with_(good, kbch_bits=3076), E, KBCH_TEXT), (with_(good, kbch_bits=80), E, KBCH_TEXT), (with_(good, n_streams=0), E, STREAMS_TEXT),
            (with_(good, n_streams=1025), E, STREAMS_TEXT), (with_(good, max_frames=0), E, FRAMES_TEXT), (with_(good, max_frames=(1 << 20) + 1), E, FRAMES_TEXT),
            (with_(good, d_bbframes=0), E, "bbframes is null"), (with_(good, d_offsets=0), E, "offsets is null"), (with_(good, d_state=0), E, "state is null"),
            (with_(good, d_work=0), E, "work is null"), (with_(good, d_ts_out=0), E, "ts_out is null"), (with_(good, d_pkt_offsets=0), E, "pkt_offsets is null"),
            (with_(good, d_offsets=D2), E, "offsets and pkt_offsets must be 4-byte aligned"), (with_(good, d_pkt_offsets=D2), E, "offsets and pkt_offsets must be 4-byte aligned"),
            (with_(good, d_state=B8), E, "state must be 16-byte aligned"), (with_(good, d_state=C4), E, "state must be 16-byte aligned"),
            (with_(good, d_work=B8), E, "work must be 16-byte aligned"), (with_(good, work_bytes=g["work_bytes"] - 1), Z, size("work_bytes")),
            (with_(good, work_bytes=0), Z, size("work_bytes")), (with_(good, work_bytes=-1), Z, size("work_bytes")),
            (with_(good, out_bytes=g["out_bytes"] - 1), Z, size("out_bytes")), (with_(good, out_bytes=0), Z, size("out_bytes")),
            # several wrong: the ranges, then the pointers in argument order, then the alignment, then the sizes
            (with_(good, n_streams=0, d_bbframes=0), E, STREAMS_TEXT), (with_(good, d_state=0, d_work=B8), E, "state is null"),
            (with_(good, d_work=B8, work_bytes=0), E, "work must be 16-byte aligned"), (with_(good, work_bytes=0, out_bytes=0), Z, size("work_bytes"))]


def rows_call(a):
    return lib.dvbs2_bbdeheader_rows_device(*[(v or None) if i in POINTERS else v for i, v in enumerate(a)], 0, None)


def rows_line(a):
    return "rows %x %d %x %d %d %x %x %d %x %d %x" % a


def work_bytes_restated(S, mf):
    a16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    return 2 * a16(4 * mf) + a16(24 * mf) + a16(24 * S)  # header words, the frame-to-stream map, the plans (six ints), one tail plan per stream


def test_check_names_the_argument():
    for a, text in CHECKS:
        assert bbdeheader_rows_check(*a) == text, a
        if text is None:
            assert lib.dvbs2_bbdeheader_rows_check(*a) == capi.OK
        else:
            T.refused(capi.EINVAL, text, lib.dvbs2_bbdeheader_rows_check, *a)


@pytest.mark.parametrize("kbch", [3072, 16008, 58192])
def test_geometry(kbch):
    """kbch_bytes and max_out_bytes_per_frame are what dvbs2_bbdeheader_params gives for a handle of this kbch (csrc/bbdeheader_hip.h,
    restated by the oracle's wrapper; tests/test_bbdeheader_rows_gpu.py compares with a live handle); out_bytes is max_frames times that
    and bounds what any headers can make a frame complete; work_bytes is the restated sum"""
    single = T.OracleBbDeheader(kbch)
    for S, mf in ((1, 1), (5, 700), (1024, 1 << 20), (3, 5)):
        g = bbdeheader_rows_geometry(kbch, S, mf)
        assert g["kbch_bytes"] == kbch // 8 == single.kbch_bytes and g["max_out_bytes_per_frame"] == single.max_out
        assert g["max_out_bytes_per_frame"] == {3072: 2, 16008: 11, 58192: 39}[kbch] * 188
        assert g["out_bytes"] == mf * g["max_out_bytes_per_frame"] and g["work_bytes"] == work_bytes_restated(S, mf) and g["work_bytes"] % 16 == 0
    # the bound: a frame completes floor((carried + dfl) / 188) packets with carried <= 187 and dfl <= max_dfl
    dflb = (kbch - 80) // 8
    assert (187 + dflb) // 188 * 188 == bbdeheader_rows_geometry(kbch, 1, 1)["max_out_bytes_per_frame"]
    # a refusal writes nothing
    v = [C.c_int(-7), C.c_int(-7), C.c_int64(-7), C.c_int64(-7)]
    T.refused(capi.EINVAL, STREAMS_TEXT, lib.dvbs2_bbdeheader_rows_geometry, kbch, 0, 1, *[C.byref(x) for x in v])
    assert [x.value for x in v] == [-7] * 4
    assert lib.dvbs2_bbdeheader_rows_geometry(kbch, 1, 1, None, None, None, None) == capi.OK


def hand_made():
    st = np.zeros(4, BBDEHEADER_STATE)
    st["synched"] = [1, 0, 1, -3]
    st["partial_ts_bytes"] = [151, 0, 187, 5]
    for i, k in enumerate(("packets", "errors", "bbframes", "dropped", "gaps", "overruns")):
        st[k] = [i + 1, 0, (1 << 64) - 1 - i, 1 << (40 + i)]
    st["last_packets"] = [9, 8, 7, 6]
    st["reserved"] = -1
    st["partial_pkt"] = 0xAB
    st["padding"] = 0xCD
    return st


def test_state_counters_on_hand_made_records():
    assert BBDEHEADER_STATE.itemsize == 256 and BBDEHEADER_STATE.fields["partial_pkt"][1] == 64 and BBDEHEADER_STATE.fields["last_packets"][1] == 56
    assert not np.zeros(1, BBDEHEADER_STATE).tobytes().strip(b"\0")  # the block as constructed is all-zero bytes
    st = hand_made()
    got = bbdeheader_state_counters(st)
    assert len(got) == 4
    for r, c in zip(st, got):
        assert c == {k: int(r[k]) for k in ("packets", "errors", "bbframes", "dropped", "gaps", "overruns", "synched", "partial_ts_bytes")}
    assert bbdeheader_state_counters(st[2:3]) == got[2:3]
    out = (capi.BbDeheaderCounters * 1)()
    T.refused(capi.EINVAL, "state is null", lib.dvbs2_bbdeheader_state_counters, None, 1, C.addressof(out))
    T.refused(capi.EINVAL, "out is null", lib.dvbs2_bbdeheader_state_counters, st.ctypes.data, 1, None)
    T.refused(capi.EINVAL, STREAMS_TEXT, lib.dvbs2_bbdeheader_state_counters, st.ctypes.data, 0, C.addressof(out))
    T.refused(capi.EINVAL, STREAMS_TEXT, lib.dvbs2_bbdeheader_state_counters, st.ctypes.data, 1025, C.addressof(out))
    assert bytes(out) == bytes(C.sizeof(out))


def test_device_entry_refusals_come_before_the_device():
    """every refusal with its code and its exact text, with addresses that are never dereferenced: a refused call reads and writes
    nothing (tests/test_bbdeheader_rows_stream_gpu.py repeats the list over live buffers and finds them unchanged)"""
    for a, code, text in rows_refused():
        T.refused(code, text, lib.dvbs2_bbdeheader_rows_device, *[(v or None) if i in POINTERS else v for i, v in enumerate(a)], 0, None)


def test_host_program_under_the_host_sanitizers(host_exe):
    rows, want = [], []
    for a, text in CHECKS:
        rows.append("check %d %d %d" % a)
        want.append("ok" if text is None else f"refused -1: {text}")
    for a, text in CHECKS:
        rows.append("geometry %d %d %d" % a)
        if text is None:
            g = bbdeheader_rows_geometry(*a)
            want.append("ok %d %d %d %d" % (g["kbch_bytes"], g["max_out_bytes_per_frame"], g["work_bytes"], g["out_bytes"]))
        else:
            want.append(f"refused -1: {text} untouched")
    st = hand_made()
    fields = ("synched", "partial_ts_bytes", "packets", "errors", "bbframes", "dropped", "gaps", "overruns")
    for recs in (st, st[1:2]):
        rows.append("counters %d %s" % (len(recs), " ".join(str(int(r[k])) for r in recs for k in fields)))
        want.append("ok " + " ".join(str(c[k]) for c in bbdeheader_state_counters(recs)
                                     for k in ("packets", "errors", "bbframes", "dropped", "gaps", "overruns", "synched", "partial_ts_bytes")))
    # the device entry: arguments that pass every check reach the device lookup, which this program answers itself
    for good in (good_rows(), good_rows(58192, 1024, 1 << 20), good_rows(88, 1, 1)):
        rows.append(rows_line(good))
        want.append("refused -2: this program looks for no device")
    for a, code, text in rows_refused():
        rows.append(rows_line(a))
        want.append(f"refused {code}: {text}")
        assert said(rows_call(a)) == want[-1]
    rows.append("null")
    want += ["counters-state -1: state is null", "counters-out -1: out is null", f"counters-none -1: {STREAMS_TEXT}", f"counters-many -1: {STREAMS_TEXT}",
             "outputs nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(want)
    for row, got, w in zip(rows + ["null"] * 4, lines, want):
        assert got == w, row
