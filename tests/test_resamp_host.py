"""CPU: the host-only code of the resampler -- step, geometry, max_out, the position rule over a sequence of calls and the argument check
of the class -- once more in a stand-alone program built with the host sanitizers, over good and refused arguments. Its answers must be
the library's, and the position rule's those of tests/resamp_model.py."""

import numpy as np
import pytest

import fec_testlib as T
import resamp_model as RM
from dvbs2rx_amd import capi, resamp_geometry, resamp_max_out, resamp_step


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/resamp_host_main.cpp with the host source it calls, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("resamp"), "resamp_host_main.cpp", ("resamp_hip.hip",))


def _hex(taps):
    return " ".join("%08x" % b for b in np.ascontiguousarray(taps, np.float32).view(np.uint32))


def _lib_refuses(nfilts, taps, rate, max_streams, max_samples):
    t = np.ascontiguousarray(taps, np.float32)
    rc = capi.lib.dvbs2_resamp_check(nfilts, t.ctypes.data if t.size else None, int(t.size), rate, max_streams, max_samples)
    assert rc == capi.EINVAL
    return capi.lib.dvbs2_last_error().decode()


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(13)
    rows, want = [], []
    good_rates = (0.5, 64.0, 1.0, 2.5, 0.8, 1 + 1e-4, 1 - 1e-4, 63.999, 0.50001, 3.0)
    bad_rates = (0.4999, 64.001, 0.0, -1.0, float("nan"), float("inf"))
    for rate in good_rates:
        rows.append(f"step {float(rate).hex()}")
        want.append(str(resamp_step(rate)))
    for rate in bad_rates:
        rows.append(f"step {float(rate).hex() if np.isfinite(rate) else rate}")
        want.append("refused")
    for nfilts, ntaps in ((2, 1), (2, 256), (256, 8192), (32, 321), (16, 401), (256, 1000), (64, 63)):
        rows.append(f"geom {nfilts} {ntaps}")
        want.append("%d %d %d" % resamp_geometry(nfilts, ntaps))
    for nfilts, ntaps in ((0, 5), (3, 5), (512, 5), (2, 0), (2, 257), (256, 8193), (-4, -1)):
        rows.append(f"geom {nfilts} {ntaps}")
        want.append("refused")
    steps = [RM.MIN_STEP, RM.MAX_STEP, 1 << 32, RM.step_of(2.5), RM.step_of(0.8), RM.step_of(1 + 1e-4)] + [int(s) | 1 for s in
                                                                                                        rng.integers(RM.MIN_STEP, RM.MAX_STEP, 6)]
    for step in steps:
        for n_in in (0, 1, 1000, RM.MAX_SAMPLES):
            rows.append(f"maxout {step} {n_in}")
            want.append(str(resamp_max_out(step, n_in)))
            assert resamp_max_out(step, n_in) == RM.max_out(step, n_in)
    for step, n_in in ((RM.MIN_STEP - 1, 5), (RM.MAX_STEP + 1, 5), (0, 5), (1 << 32, -1), (1 << 32, RM.MAX_SAMPLES + 1)):
        rows.append(f"maxout {step} {n_in}")
        want.append("refused")
    # the position rule over sequences of calls, zeros and the largest call included, against the model's Python integers
    for step in steps:
        for acc in (0, (1 << 32) - 1, int(rng.integers(0, 1 << 32))):
            cuts = [int(c) for c in rng.integers(0, 5000, 5)] + [0, 1, RM.MAX_SAMPLES, 0]
            rng.shuffle(cuts)
            rows.append(f"produce {step} {acc} {len(cuts)} " + " ".join(map(str, cuts)))
            line = []
            for n_in in cuts:
                n, acc = RM.advance(acc, step, n_in)
                line += [str(n), str(acc)]
            want.append(" ".join(line))
    # the argument check of the class: the longest accepted filters, then every refusal a row can express
    for nfilts, rate, taps in ((2, 1.0, rng.normal(size=256)), (256, 64.0, rng.normal(size=8192)), (4, 0.5, rng.normal(size=1)),
                               (32, 2.5, rng.normal(size=321))):
        rows.append(f"check {nfilts} {float(rate).hex()} 1 16 {len(taps)} {_hex(taps)}")
        want.append("ok")
    nonfinite = rng.normal(size=21)
    nonfinite[20] = np.inf
    for nfilts, rate, ms, mx, taps in ((3, 1.0, 1, 16, np.ones(3)), (512, 1.0, 1, 16, np.ones(3)), (2, 1.0, 1, 16, rng.normal(size=257)),
                                       (256, 1.0, 1, 16, rng.normal(size=8193)), (2, 1.0, 1, 16, np.ones(0)), (2, 1.0, 1, 16, nonfinite),
                                       (2, 0.25, 1, 16, np.ones(3)), (2, 65.0, 1, 16, np.ones(3)), (2, 1.0, 0, 16, np.ones(3)),
                                       (2, 1.0, 65536, 16, np.ones(3)), (2, 1.0, 1, 0, np.ones(3)), (2, 1.0, 1, (1 << 24) + 1, np.ones(3))):
        rows.append(f"check {nfilts} {float(rate).hex()} {ms} {mx} {len(taps)} {_hex(taps)}")
        want.append("refused: " + _lib_refuses(nfilts, taps, rate, ms, mx))
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows)
    for row, got, w in zip(rows, lines, want):
        assert got == w, row[:60]
    assert sum(w.startswith("refused") for w in want) == len(bad_rates) + 7 + 5 + 12
