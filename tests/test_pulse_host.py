"""CPU: the host-only code of the pulse shaper -- geometry, tap design, tap scaling and the argument check of the class -- once more in a
stand-alone program built with the host sanitizers, over good and refused arguments. Its tap values must be the library's, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import capi, pulse_geometry, pulse_scale_taps, pulse_taps


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/pulse_host_main.cpp with the host source it calls, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("pulse"), "pulse_host_main.cpp", ("pulse_hip.hip",))


def _hex(taps):
    return " ".join("%08x" % b for b in np.ascontiguousarray(taps, np.float32).view(np.uint32))


def _lib_refuses_create(sps, taps, max_streams, max_symbols):
    h = C.c_void_p()
    t = np.ascontiguousarray(taps, np.float32)
    rc = capi.lib.dvbs2_pulse_create_taps(C.byref(h), sps, t.ctypes.data if t.size else None, int(t.size), max_streams, max_symbols, 0)
    assert rc == capi.EINVAL and not h  # every row below is refused before a device is looked for
    return capi.lib.dvbs2_last_error().decode()


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(12)
    rows, want = [], []
    # geometry: the corners and what lies outside them
    for sps, delay in ((2, 1), (2, 64), (64, 1), (64, 64), (6, 3), (4, 5)):
        rows.append(f"geom {sps} {delay}")
        want.append("%d %d %d" % pulse_geometry(sps, delay))
    for sps, delay in ((0, 5), (3, 5), (66, 5), (2, 0), (2, 65), (-4, -1)):
        rows.append(f"geom {sps} {delay}")
        want.append("refused")
    # designed taps: the longest design, the singular points (rolloff 0.25 at sps 4), both ends of rolloff and tau
    for sps, rolloff, delay, tau, gain in ((2, 0.2, 5, 0.0, 2.0), (4, 0.2, 5, 0.3, 4.0), (64, 0.35, 64, -0.5, 64.0), (4, 0.25, 5, 0.0, 1.0),
                                           (2, 0.0, 3, 0.5, -1.5), (8, 1.0, 2, 0.125, 8.0), (6, 0.05, 3, -0.25, 0.001)):
        rows.append(f"taps {sps} {rolloff!r} {delay} {tau!r} {gain!r}")
        want.append(_hex(pulse_taps(sps, rolloff, delay, tau, gain)))
    for sps, rolloff, delay, tau, gain in ((3, 0.2, 5, 0.0, 1.0), (2, 0.2, 65, 0.0, 1.0), (2, 1.25, 5, 0.0, 1.0), (2, -0.5, 5, 0.0, 1.0),
                                           (2, 0.2, 5, 0.625, 1.0), (2, 0.2, 5, -0.75, 1.0), (2, 0.2, 5, 0.0, 0.0)):
        rows.append(f"taps {sps} {rolloff!r} {delay} {tau!r} {gain!r}")
        want.append("refused")
    # scaling: designed taps, random ones, fewer taps than phases, one tap
    for sps, taps, fullscale in ((2, pulse_taps(2, 0.2, 5), 1.0), (4, pulse_taps(4, 0.35, 5, 0.3), 0.5), (6, rng.normal(size=37), 32767.0),
                                 (4, rng.normal(size=3), 1.0), (64, rng.normal(size=1), 2.0), (1, rng.normal(size=5), 1.0)):
        rows.append(f"scale {sps} {fullscale!r} {len(taps)} {_hex(taps)}")
        want.append(_hex(pulse_scale_taps(np.asarray(taps, np.float32), sps, fullscale)))
    for sps, taps, fullscale in ((2, np.zeros(4), 1.0), (0, np.ones(4), 1.0), (2, np.ones(0), 1.0), (2, np.array([1, np.inf, 1]), 1.0),
                                 (2, np.array([np.nan]), 1.0)):
        rows.append(f"scale {sps} {fullscale!r} {len(taps)} {_hex(taps)}")
        want.append("refused")
    # the argument check of the class: the longest accepted filter at both ends of sps, then every refusal
    for sps, taps in ((2, rng.normal(size=258)), (64, rng.normal(size=129 * 64)), (4, rng.normal(size=1)), (6, pulse_taps(6, 0.2, 3))):
        rows.append(f"check {sps} 1 16 {len(taps)} {_hex(taps)}")
        want.append("ok")
    nonfinite = rng.normal(size=21)
    nonfinite[20] = np.inf
    for sps, ms, mx, taps in ((2, 1, 16, rng.normal(size=259)), (64, 1, 16, rng.normal(size=129 * 64 + 1)), (2, 1, 16, np.ones(0)),
                              (5, 1, 16, np.ones(3)), (66, 1, 16, np.ones(3)), (2, 1, 16, nonfinite), (2, 0, 16, np.ones(3)),
                              (2, 65536, 16, np.ones(3)), (2, 1, 0, np.ones(3)), (2, 1, (1 << 30) + 1, np.ones(3))):
        rows.append(f"check {sps} {ms} {mx} {len(taps)} {_hex(taps)}")
        want.append("refused: " + _lib_refuses_create(sps, taps, ms, mx))
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows)
    for row, got, w in zip(rows, lines, want):
        assert got == w, row[:60]
    assert sum(w.startswith("refused") for w in want) == 6 + 7 + 5 + 10
