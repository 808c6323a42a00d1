"""CPU: the host-only code of the polyphase synthesizer -- geometry, the tile rule, the counter over sequences of calls up to 2^54, every
refusal of the argument checks with its code and text (the n_chan * ceil(ntaps / interp) limit at both sides of its edge), and the answers
to a null handle -- once more in a stand-alone program built with the host sanitizers. Its answers must be the library's and those of
tests/pfbsyn_model.py."""

import numpy as np
import pytest

import fec_testlib as T
import pfbsyn_model as SY
from dvbs2rx_amd import capi, pfbsyn_geometry, pfbsyn_tile

SOURCES = ("c_api_pfbsyn.hip", "pfbsyn_hip.hip")  # the entries' translation unit and what it binds

PRODUCT = "n_chan * ceil(ntaps / interp) must not exceed 8192"


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/pfbsyn_host_main.cpp with the sources behind the entries, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("pfbsyn"), "pfbsyn_host_main.cpp", SOURCES)


def _hex(taps):
    return " ".join("%08x" % b for b in np.ascontiguousarray(taps, np.float32).view(np.uint32))


def _lib_refuses(M, L, taps, ms, mn):
    t = np.ascontiguousarray(taps, np.float32)
    rc = capi.lib.dvbs2_pfbsyn_check(M, L, t.ctypes.data if t.size else None, int(t.size), ms, mn)
    assert rc == capi.EINVAL
    return capi.lib.dvbs2_last_error().decode()


BAD_CHECK_TEXTS = ["n_chan must be a power of two in 2..256"] * 5 + ["interp must be in 1..n_chan"] * 3 + ["ntaps must be in 1..4096"] * 2 + \
    ["null taps", "taps[20] is not finite", "taps[0] is not finite"] + [PRODUCT] * 4 + ["max_streams out of range (1..65535)"] * 2 + \
    ["max_samples out of range (1..2^24)"] * 2 + ["max_samples * interp must not exceed 2^28"] * 2


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(23)
    rows, want = [], []
    good_geom = ((2, 1, 1), (2, 2, 4096), (256, 256, 4096), (256, 1, 1), (8, 3, 40), (8, 4, 65), (64, 32, 1025), (16, 16, 15), (32, 31, 33),
                 (256, 128, 4096), (256, 1, 32), (2, 1, 4096), (8, 1, 1024), (256, 24, 257))
    bad_geom = ((1, 1, 5), (3, 1, 5), (512, 4, 5), (0, 1, 5), (-8, 1, 5), (8, 0, 5), (8, 9, 5), (8, -1, 5), (8, 4, 0), (8, 4, 4097))
    for M, L, ntaps in good_geom:
        rows.append(f"geom {M} {L} {ntaps}")
        want.append("%d %d %d" % pfbsyn_geometry(M, L, ntaps))
        assert pfbsyn_geometry(M, L, ntaps) == SY.geometry(M, L, ntaps)
        rows.append(f"tile {M} {L} {ntaps}")
        want.append(str(pfbsyn_tile(M, L, ntaps)))
        assert pfbsyn_tile(M, L, ntaps) == SY.tile(M, L, ntaps) and SY.lds_bytes(M, L, ntaps) <= 120 * 1024
    for M, L, ntaps in bad_geom:
        rows.append(f"geom {M} {L} {ntaps}")
        want.append("refused")
        with pytest.raises(capi.Dvbs2Error):
            pfbsyn_geometry(M, L, ntaps)
    # the tile rule at the edge of the product limit: the last shape that is accepted and the first that is not
    edge = ((256, 1, 32, 33), (256, 128, 4096, None), (256, 127, 4064, 4065), (8, 1, 1024, 1025), (2, 1, 4096, None), (128, 3, 192, 193))
    n_tile_refused = 0
    for M, L, ok, over in edge:
        assert SY.legal(M, L, ok) and M * -(-ok // L) == SY.MAX_PRODUCT
        rows.append(f"tile {M} {L} {ok}")
        want.append(str(SY.tile(M, L, ok)))
        if over is not None:
            assert not SY.legal(M, L, over)
            rows.append(f"tile {M} {L} {over}")
            want.append(f"refused {capi.EINVAL}: {PRODUCT}")
            n_tile_refused += 1
    # sequences of calls against Python integers: from zero, and up to 2^54 exactly; one step further is refused
    n_seq_refused = 0
    for start in (0, SY.MAX_POSITION - 3 * SY.MAX_SAMPLES - 7):
        calls = [int(c) for c in rng.integers(0, 5000, 5)] + [0, 1, SY.MAX_SAMPLES]
        rng.shuffle(calls)
        if start:
            calls += [SY.MAX_SAMPLES, 0]
            calls += [SY.MAX_POSITION - start - sum(calls), 0, 1, 5]  # lands on 2^54; an empty call is still fine there, one instant is not
        rows.append(f"seq {start} {len(calls)} " + " ".join(map(str, calls)))
        counter, line = start, []
        for n_in in calls:
            nxt = SY.advance(counter, n_in)
            if nxt is None:
                line.append("refused")
                n_seq_refused += 1
                break
            counter = nxt
            line.append(str(counter))
        assert not start or (counter == SY.MAX_POSITION and line[-1] == "refused" and line[-2] == line[-3] == str(SY.MAX_POSITION))
        want.append(" ".join(line))
    for position, n_in in ((-1, 5), (SY.MAX_POSITION + 1, 0), (0, -1), (0, SY.MAX_SAMPLES + 1), (SY.MAX_POSITION, 1)):
        assert SY.advance(position, n_in) is None
        rows.append(f"seq {position} 1 {n_in}")
        want.append("refused")
        n_seq_refused += 1
    assert n_seq_refused == 6
    # the argument check: accepted corners, then every refusal with its text; create refuses the same with the same code before it
    # looks for a device
    good_check = ((2, 1, 1, 1, rng.normal(size=1)), (256, 256, 65535, 1 << 20, rng.normal(size=4096)), (8, 3, 2, 4096, rng.normal(size=40)),
                  (256, 1, 1, 1 << 24, rng.normal(size=32)), (256, 127, 1, 16, rng.normal(size=4064)), (8, 8, 1, 1 << 24, rng.normal(size=3)),
                  (2, 1, 1, 16, rng.normal(size=4096)), (16, 16, 1, 1 << 24, rng.normal(size=3)))
    for M, L, ms, mn, taps in good_check:
        rows.append(f"check {M} {L} {ms} {mn} {len(taps)} {_hex(taps)}")
        want.append("ok")
    nonfinite, nan0 = rng.normal(size=21), np.ones(3)
    nonfinite[20], nan0[0] = np.inf, np.nan
    ones = np.ones(3)
    bad_check = ((0, 1, 1, 16, ones), (1, 1, 1, 16, ones), (6, 2, 1, 16, ones), (512, 2, 1, 16, ones), (-8, 2, 1, 16, ones),
                 (8, 0, 1, 16, ones), (8, 9, 1, 16, ones), (8, -3, 1, 16, ones), (8, 4, 1, 16, np.ones(0)), (8, 4, 1, 16, rng.normal(size=4097)),
                 None, (8, 4, 1, 16, nonfinite), (8, 4, 1, 16, nan0),
                 (256, 1, 1, 16, np.ones(33)), (256, 127, 1, 16, np.ones(4065)), (8, 1, 1, 16, np.ones(1025)), (4, 1, 1, 16, np.ones(2049)),
                 (8, 4, 0, 16, ones), (8, 4, 65536, 16, ones), (8, 4, 1, 0, ones), (8, 4, 1, (1 << 24) + 1, ones),
                 (32, 32, 1, (1 << 23) + 1, ones), (256, 17, 1, 1 << 24, ones))
    assert len(bad_check) == len(BAD_CHECK_TEXTS)
    for i, case in enumerate(bad_check):
        if case is None:  # null taps with a good count: only the C side can say it
            assert capi.lib.dvbs2_pfbsyn_check(8, 4, None, 3, 1, 16) == capi.EINVAL and capi.lib.dvbs2_last_error().decode() == BAD_CHECK_TEXTS[i]
            continue
        M, L, ms, mn, taps = case
        text = _lib_refuses(M, L, taps, ms, mn)
        assert text == BAD_CHECK_TEXTS[i], (case[:4], text)
        for what in ("check", "create"):
            rows.append(f"{what} {M} {L} {ms} {mn} {len(taps)} {_hex(taps)}")
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
    assert sum(w.startswith("refused") or w.endswith("refused") for w in want) == len(bad_geom) + n_tile_refused + n_seq_refused + 2 * (len(bad_check) - 1) + 1 + len(bad_lists)
