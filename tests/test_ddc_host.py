"""CPU: the host-only code of the digital down-converter -- geometry, the count rule, the tile rule, the counter and phase mirror over
sequences of calls and the argument check of the class -- once more in a stand-alone program built with the host sanitizers, over good
and refused arguments. Its answers must be the library's and those of tests/ddc_model.py."""

import numpy as np
import pytest

import ddc_model as DM
import fec_testlib as T
from dvbs2rx_amd import capi, ddc_geometry, ddc_produce, ddc_tile


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/ddc_host_main.cpp with the host source it calls, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("ddc"), "ddc_host_main.cpp", ("ddc_hip.hip",))


def _hex(taps):
    return " ".join("%08x" % b for b in np.ascontiguousarray(taps, np.float32).view(np.uint32))


def _lib_refuses(decim, taps, mc, mi, ms):
    t = np.ascontiguousarray(taps, np.float32)
    rc = capi.lib.dvbs2_ddc_check(decim, t.ctypes.data if t.size else None, int(t.size), mc, mi, ms)
    assert rc == capi.EINVAL
    return capi.lib.dvbs2_last_error().decode()


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(17)
    rows, want = [], []
    good_geom = ((1, 1), (1, 4096), (256, 1), (256, 4096), (8, 129), (50, 801), (3, 2))
    bad_geom = ((0, 5), (257, 5), (-1, 5), (4, 0), (4, 4097), (-4, -1))
    for D, ntaps in good_geom:
        rows.append(f"geom {D} {ntaps}")
        want.append("%d %d" % ddc_geometry(D, ntaps))
        assert ddc_geometry(D, ntaps) == DM.geometry(D, ntaps)
        rows.append(f"tile {D} {ntaps}")
        want.append(str(ddc_tile(D, ntaps)))
        assert ddc_tile(D, ntaps) == DM.tile(D, ntaps)
    for D, ntaps in bad_geom:
        rows.append(f"geom {D} {ntaps}")
        want.append("refused")
    for D in (1, 2, 3, 8, 255, 256):
        for position in (0, 1, D - 1, D, 987654321, DM.MAX_POSITION):
            for n_in in (0, 1, D - 1, D, 1000, DM.MAX_SAMPLES):
                rows.append(f"produce {position} {D} {n_in}")
                want.append(str(ddc_produce(position, D, n_in)))
                assert ddc_produce(position, D, n_in) == DM.produce(position, D, n_in)
    bad_produce = ((-1, 4, 5), (DM.MAX_POSITION + 1, 4, 5), (0, 0, 5), (0, 257, 5), (0, 4, -1), (0, 4, DM.MAX_SAMPLES + 1))
    for position, D, n_in in bad_produce:
        rows.append(f"produce {position} {D} {n_in}")
        want.append("refused")
    # the mirror over sequences of calls, zeros, the largest call and calls on some of the channels included, against Python integers
    for D in (1, 3, 8, 256):
        nch = 3
        incs = [0, (1 << 64) - 1, int(rng.integers(0, 1 << 63)) * 2 + 1]
        calls = [(int(c), int(rng.integers(0, nch + 1))) for c in rng.integers(0, 5000, 5)] + [(0, nch), (1, nch), (DM.MAX_SAMPLES, nch), (D - 1, 1)]
        rng.shuffle(calls)
        rows.append(f"mirror {D} {nch} " + " ".join(map(str, incs)) + f" {len(calls)} " + " ".join(f"{a} {b}" for a, b in calls))
        counter, phases, line = 0, [0] * nch, []
        for n_in, n_channels in calls:
            line.append(str(DM.produce(counter, D, n_in)))
            phases = [DM.phase_after(p, incs[c], n_in) if c < n_channels else p for c, p in enumerate(phases)]
            counter += n_in
            line += [str(counter)] + [str(p) for p in phases]
        want.append(" ".join(line))
    # the argument check of the class: the longest accepted filter, then every refusal a row can express
    for D, mc, mi, ms, taps in ((1, 1, 1, 1, rng.normal(size=1)), (256, 65535, 65535, 1 << 24, rng.normal(size=4096)), (8, 16, 2, 4096, rng.normal(size=129))):
        rows.append(f"check {D} {mc} {mi} {ms} {len(taps)} {_hex(taps)}")
        want.append("ok")
    nonfinite = rng.normal(size=21)
    nonfinite[20] = np.inf
    bad_check = ((0, 1, 1, 16, np.ones(3)), (257, 1, 1, 16, np.ones(3)), (4, 1, 1, 16, np.ones(0)), (4, 1, 1, 16, rng.normal(size=4097)),
                 (4, 1, 1, 16, nonfinite), (4, 0, 1, 16, np.ones(3)), (4, 65536, 1, 16, np.ones(3)), (4, 1, 0, 16, np.ones(3)),
                 (4, 1, 65536, 16, np.ones(3)), (4, 1, 1, 0, np.ones(3)), (4, 1, 1, (1 << 24) + 1, np.ones(3)))
    for D, mc, mi, ms, taps in bad_check:
        rows.append(f"check {D} {mc} {mi} {ms} {len(taps)} {_hex(taps)}")
        want.append("refused: " + _lib_refuses(D, taps, mc, mi, ms))
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows)
    for row, got, w in zip(rows, lines, want):
        assert got == w, row[:60]
    assert sum(w.startswith("refused") for w in want) == len(bad_geom) + len(bad_produce) + len(bad_check)
