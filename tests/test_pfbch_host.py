"""CPU: the host-only code of the polyphase channelizer -- geometry, the count rule over sequences of calls up to a counter of 2^62, the
tile rule, the twiddle table, every refusal of the argument checks with its code and text, and the answers to a null handle -- once more
in a stand-alone program built with the host sanitizers. Its answers must be the library's and those of tests/pfbch_model.py."""

import numpy as np
import pytest

import fec_testlib as T
import pfbch_model as PM
from dvbs2rx_amd import capi, pfbch_geometry, pfbch_produce, pfbch_tile, pfbch_twiddles

SOURCES = ("c_api_pfbch.hip", "pfbch_hip.hip")  # the entries' translation unit and what it binds


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/pfbch_host_main.cpp with the sources behind the entries, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("pfbch"), "pfbch_host_main.cpp", SOURCES)


def _hex(taps):
    return " ".join("%08x" % b for b in np.ascontiguousarray(taps, np.float32).view(np.uint32))


def _lib_refuses(M, D, taps, ms, mn):
    t = np.ascontiguousarray(taps, np.float32)
    rc = capi.lib.dvbs2_pfbch_check(M, D, t.ctypes.data if t.size else None, int(t.size), ms, mn)
    assert rc == capi.EINVAL
    return capi.lib.dvbs2_last_error().decode()


BAD_CHECK_TEXTS = ["n_chan must be a power of two in 2..256"] * 5 + ["decim must be in 1..n_chan"] * 3 + ["ntaps must be in 1..4096"] * 2 + \
    ["null taps", "taps[20] is not finite", "taps[0] is not finite"] + ["max_streams out of range (1..65535)"] * 2 + ["max_samples out of range (1..2^24)"] * 2


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(23)
    rows, want = [], []
    good_geom = ((2, 1, 1), (2, 2, 4096), (256, 256, 4096), (256, 1, 1), (8, 3, 40), (8, 4, 65), (64, 32, 1025), (16, 16, 15), (32, 31, 33))
    bad_geom = ((1, 1, 5), (3, 1, 5), (512, 4, 5), (0, 1, 5), (-8, 1, 5), (8, 0, 5), (8, 9, 5), (8, -1, 5), (8, 4, 0), (8, 4, 4097))
    for M, D, ntaps in good_geom:
        rows.append(f"geom {M} {D} {ntaps}")
        want.append("%d %d %d" % pfbch_geometry(M, D, ntaps))
        assert pfbch_geometry(M, D, ntaps) == PM.geometry(M, D, ntaps)
        rows.append(f"tile {M} {D} {ntaps}")
        want.append(str(pfbch_tile(M, D, ntaps)))
        assert pfbch_tile(M, D, ntaps) == PM.tile(M, D, ntaps)
    for M, D, ntaps in bad_geom:
        rows.append(f"geom {M} {D} {ntaps}")
        want.append("refused")
        with pytest.raises(capi.Dvbs2Error):
            pfbch_geometry(M, D, ntaps)
    for D in (1, 2, 3, 8, 255, 256):
        for position in (0, 1, D - 1, D, 987654321, PM.MAX_POSITION):
            for n_in in (0, 1, D - 1, D, 1000, PM.MAX_SAMPLES):
                rows.append(f"produce {position} {D} {n_in}")
                want.append(str(pfbch_produce(position, D, n_in)))
                assert pfbch_produce(position, D, n_in) == PM.produce(position, D, n_in)
    bad_produce = ((-1, 4, 5), (PM.MAX_POSITION + 1, 4, 5), (0, 0, 5), (0, 257, 5), (0, 4, -1), (0, 4, PM.MAX_SAMPLES + 1))
    for position, D, n_in in bad_produce:
        rows.append(f"produce {position} {D} {n_in}")
        want.append("refused")
    # sequences of calls against Python integers: from zero, and up to the last counter a call may start from; one step further is refused
    n_seq_refused = 0
    for D in (1, 3, 8, 256):
        for start in (0, PM.MAX_POSITION - 3 * PM.MAX_SAMPLES):
            calls = [int(c) for c in rng.integers(0, 5000, 5)] + [0, 1, D - 1, PM.MAX_SAMPLES, PM.MAX_SAMPLES]
            rng.shuffle(calls)
            calls += [PM.MAX_SAMPLES, 7] if start else []
            rows.append(f"seq {start} {D} {len(calls)} " + " ".join(map(str, calls)))
            counter, line = start, []
            for n_in in calls:
                if counter > PM.MAX_POSITION:
                    line.append("refused")
                    n_seq_refused += 1
                    break
                line += [str(PM.produce(counter, D, n_in)), str(counter + n_in)]
                counter += n_in
            want.append(" ".join(line))
    assert n_seq_refused == 4
    for M in (2, 4, 8, 16, 32, 64, 128, 256):
        rows.append(f"tw {M}")
        want.append(_hex(pfbch_twiddles(M).view(np.float32)))
    bad_tw = (0, 1, 3, 48, 512, -4)
    for M in bad_tw:
        rows.append(f"tw {M}")
        want.append("refused")
    # the argument check: accepted corners, then every refusal with its text; create refuses the same with the same code before it
    # looks for a device
    for M, D, ms, mn, taps in ((2, 1, 1, 1, rng.normal(size=1)), (256, 256, 65535, 1 << 24, rng.normal(size=4096)), (8, 3, 2, 4096, rng.normal(size=40))):
        rows.append(f"check {M} {D} {ms} {mn} {len(taps)} {_hex(taps)}")
        want.append("ok")
    nonfinite, nan0 = rng.normal(size=21), np.ones(3)
    nonfinite[20], nan0[0] = np.inf, np.nan
    ones = np.ones(3)
    bad_check = ((0, 1, 1, 16, ones), (1, 1, 1, 16, ones), (6, 2, 1, 16, ones), (512, 2, 1, 16, ones), (-8, 2, 1, 16, ones),
                 (8, 0, 1, 16, ones), (8, 9, 1, 16, ones), (8, -3, 1, 16, ones), (8, 4, 1, 16, np.ones(0)), (8, 4, 1, 16, rng.normal(size=4097)),
                 None, (8, 4, 1, 16, nonfinite), (8, 4, 1, 16, nan0), (8, 4, 0, 16, ones), (8, 4, 65536, 16, ones), (8, 4, 1, 0, ones),
                 (8, 4, 1, (1 << 24) + 1, ones))
    for i, case in enumerate(bad_check):
        if case is None:  # null taps with a good count: only the C side can say it
            assert capi.lib.dvbs2_pfbch_check(8, 4, None, 3, 1, 16) == capi.EINVAL and capi.lib.dvbs2_last_error().decode() == BAD_CHECK_TEXTS[i]
            continue
        M, D, ms, mn, taps = case
        text = _lib_refuses(M, D, taps, ms, mn)
        assert text == BAD_CHECK_TEXTS[i], (case[:4], text)
        for what in ("check", "create"):
            rows.append(f"{what} {M} {D} {ms} {mn} {len(taps)} {_hex(taps)}")
            want.append(f"refused {capi.EINVAL}: {text}")
    rows.append(f"create 8 4 1 16 3 {_hex(ones)}")  # good arguments: refused where the device is looked for
    want.append(f"refused {capi.EDEVICE}: this program looks for no device")
    good_lists = ((8, [0]), (8, [7, 0, 3]), (8, list(range(8))), (2, [1, 0]), (256, list(range(255, -1, -1))))
    bad_lists = ((8, -2, [], "null list"), (8, 0, [], "n_sel must be in 1..n_chan"), (8, 9, list(range(9)), "n_sel must be in 1..n_chan"),
                 (8, 2, [0, 8], "list[1] is not a channel"), (8, 1, [-1], "list[0] is not a channel"), (8, 3, [5, 2, 5], "list[2] repeats a channel"))
    for M, sel in good_lists:
        rows.append(f"channels {M} {len(sel)} " + " ".join(map(str, sel)))
        want.append("ok")
    for M, n, sel, text in bad_lists:
        rows.append(f"channels {M} {n} " + " ".join(map(str, sel)))
        want.append("refused: " + text)
    rows.append("null")
    null_lines = [f"{e} {capi.EINVAL}: null handle" for e in ("reset", "set_channels", "params", "position", "channels", "process_device", "process")]
    null_lines += [f"create {capi.EINVAL}: null handle pointer", "destroy nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows) - 1 + len(null_lines)
    for row, got, w in zip(rows[:-1], lines, want):
        assert got == w, (row[:60], got[:80], w[:80])
    assert lines[len(rows) - 1:] == null_lines
    assert sum(w.startswith("refused") for w in want) == len(bad_geom) + len(bad_produce) + len(bad_tw) + 2 * (len(bad_check) - 1) + 1 + len(bad_lists)
