"""CPU: the host-only code of the spectrum stage -- geometry, the windows, the twiddle table, the argument check of the class and the
carrier finder -- once more in a stand-alone program built with the host sanitizers, over good and refused arguments. Its answers must
be the library's (bit for bit) and those of tests/spectrum_model.py."""

import numpy as np
import pytest

import fec_testlib as T
import spectrum_model as SM
from dvbs2rx_amd import capi, spectrum_carriers, spectrum_geometry, spectrum_twiddles, spectrum_window


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/spectrum_host_main.cpp with the host sources it calls, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("spectrum"), "spectrum_host_main.cpp", ("spectrum_hip.hip", "spectrum_carriers.cpp"))


def _hex(values):
    return " ".join("%08x" % b for b in np.ascontiguousarray(values, np.float32).view(np.uint32))


def _lib_refuses_create(nfft, hop, avg, window, ms, mx):
    w = None if window is None else np.ascontiguousarray(window, np.float32)
    assert capi.lib.dvbs2_spectrum_check(nfft, hop, avg, None if w is None else w.ctypes.data, ms, mx) == capi.EINVAL
    return capi.lib.dvbs2_last_error().decode()


def _carrier_line(recs, n):
    out = [str(n)]
    for r in recs:
        out += ["%016x" % np.float64(r[k]).view(np.uint64) for k in ("centre", "bandwidth", "level", "floor")] + [str(r["lo_bin"]), str(r["hi_bin"])]
    return " ".join(out)


def test_host_program_under_the_host_sanitizers(host_exe):
    rng = np.random.default_rng(23)
    rows, want = [], []
    n_refused = 0
    for nfft, hop, avg, n_in in ((64, 32, 0, 0), (64, 32, 0, 63), (64, 32, 0, 64), (8192, 4096, 0, 1 << 24), (1024, 37, 17, 5000), (256, 261, 2, 4000),
                                 (64, 1, 1, 1 << 24), (64, 1 << 24, 16, 1 << 24)):
        rows.append(f"geom {nfft} {hop} {avg} {n_in}")
        want.append("%d %d %d" % spectrum_geometry(nfft, hop, avg, n_in))
        assert spectrum_geometry(nfft, hop, avg, n_in) == SM.geometry(nfft, hop, avg, n_in)
    for bad in ((96, 32, 0, 100), (32, 16, 0, 100), (16384, 32, 0, 100), (64, 0, 0, 100), (64, (1 << 24) + 1, 0, 100), (64, 32, -1, 100), (64, 32, 0, -1),
                (64, 32, 0, (1 << 24) + 1)):
        rows.append("geom %d %d %d %d" % bad)
        want.append("refused")
        n_refused += 1
    for nfft in (64, 512, 8192):
        for kind in range(4):
            rows.append(f"window {kind} {nfft}")
            want.append(_hex(spectrum_window(kind, nfft)))
        rows.append(f"twiddles {nfft}")
        want.append(_hex(spectrum_twiddles(nfft).view(np.float32)))
    for row in ("window 4 64", "window -1 64", "window 1 100", "window 1 16384", "twiddles 0", "twiddles 48", "twiddles 16384"):
        rows.append(row)
        want.append("refused")
        n_refused += 1
    # the argument check of the class: accepted corners, then every refusal a row can express
    for nfft, hop, avg, ms, mx, w in ((64, 1, 0, 1, 1, None), (8192, 1 << 24, 1 << 30, 65535, 1 << 24, rng.normal(size=8192)), (1024, 512, 16, 3, 5000, np.ones(1024))):
        rows.append(f"check {nfft} {hop} {avg} {ms} {mx} {0 if w is None else len(w)} {'' if w is None else _hex(w)}")
        want.append("ok")
    nonfinite = rng.normal(size=64)
    nonfinite[63] = np.nan
    for nfft, hop, avg, ms, mx, w in ((100, 32, 0, 1, 100, None), (32, 32, 0, 1, 100, None), (16384, 32, 0, 1, 100, None), (64, 0, 0, 1, 100, None),
                                      (64, (1 << 24) + 1, 0, 1, 100, None), (64, 32, -1, 1, 100, None), (64, 32, 0, 1, 100, nonfinite),
                                      (64, 32, 0, 1, 100, np.zeros(64)), (64, 32, 0, 0, 100, None), (64, 32, 0, 65536, 100, None), (64, 32, 0, 1, 0, None),
                                      (64, 32, 0, 1, (1 << 24) + 1, None)):
        rows.append(f"check {nfft} {hop} {avg} {ms} {mx} {0 if w is None else len(w)} {'' if w is None else _hex(w)}")
        want.append("refused: " + _lib_refuses_create(nfft, hop, avg, w, ms, mx))
        n_refused += 1
    # the carrier finder: rows with one, two and three carriers, one across the band edge, a flat row; both bin orders
    cases = []
    for centres, rs, rolloff in (((0.1,), 1 / 8, 0.2), ((-0.3, 0.22), 1 / 8, 0.35), ((0.49,), 1 / 16, 0.2), ((-0.3, 0.0, 0.3), 1 / 16, 0.35), ((), 1 / 8, 0.2)):
        row = 1.0 + 0.05 * rng.random(1024)
        for c in centres:
            row = row + SM.raised_cosine_psd(1024, c, rs, rolloff, 9.0, 0.0)
        cases.append(row.astype(np.float32))
    for row in cases:
        for shifted in (1, 0):
            r = row if shifted else np.fft.ifftshift(row)
            for params in (SM.DEFAULTS, dict(smooth=1, floor_quantile=0.5, threshold_db=3.0, min_gap=1, min_width=1)):
                rows.append("carriers %d %d %r %r %d %d %d %s" % (shifted, params["smooth"], params["floor_quantile"], params["threshold_db"], params["min_gap"],
                                                                params["min_width"], r.size, _hex(r)))
                recs, n = spectrum_carriers(r, bool(shifted), 64, **params)
                want.append(_carrier_line(recs, n))
                model = SM.carriers(r, bool(shifted), **params)
                assert n == len(model) and [(m["lo_bin"], m["hi_bin"]) for m in model] == [(int(q["lo_bin"]), int(q["hi_bin"])) for q in recs]
    assert any(w.startswith("3 ") for w in want) and any(w == "0" for w in want)
    negative = cases[0].copy()
    negative[5] = -1.0
    for head, r, text in (("1 9 0.25 6.0 4 8", negative, "psd[5] is negative or not finite"), ("1 8 0.25 6.0 4 8", cases[0], "smooth must be odd and in 1..nfft/2"),
                          ("1 9 1.25 6.0 4 8", cases[0], "floor_quantile must be in 0..1"), ("1 9 0.25 -1.0 4 8", cases[0], "threshold_db must be above 0 and at most 200"),
                          ("1 9 0.25 6.0 0 8", cases[0], "min_gap must be in 1..nfft"), ("1 9 0.25 6.0 4 2000", cases[0], "min_width must be in 1..nfft"),
                          ("1 9 0.25 6.0 4 8", cases[0][:1000], "nfft must be a power of two in 16..2^20")):
        rows.append(f"carriers {head} {r.size} {_hex(r)}")
        want.append("refused: " + text)
        n_refused += 1
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows)
    for row, got, w in zip(rows, lines, want):
        assert got == w, row[:60]
    assert sum(w.startswith("refused") for w in want) == n_refused
