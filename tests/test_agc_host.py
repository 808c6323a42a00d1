"""CPU: the host-only side of the AGC's C ABI -- dvbs2_agc_check at the corners of every refusal, the argument checks of create, and
every new entry with a null handle -- once more in a stand-alone program built with the host sanitizers. Its answers must be the
library's own. Nothing is loaded into Python by the program and no GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import capi

SOURCES = ("c_api_agc.hip", "agc_hip.hip")  # the entries' translation unit and what it binds


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/agc_host_main.cpp with the sources behind the entries, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("agc"), "agc_host_main.cpp", SOURCES)


def _hex(*values):
    return " ".join("%08x" % b for b in np.array(values, np.float32).view(np.uint32))


def _lib_check(args):
    rc = capi.lib.dvbs2_agc_check(*[float(np.float32(a)) for a in args])
    return "ok" if rc == capi.OK else f"refused {rc}: {capi.lib.dvbs2_last_error().decode()}"


def _lib_refuses_create(args, max_streams, max_samples):
    h = C.c_void_p()
    rc = capi.lib.dvbs2_agc_create(C.byref(h), *[float(np.float32(a)) for a in args], max_streams, max_samples, 0)
    assert rc == capi.EINVAL and not h  # every row below is refused before a device is looked for
    return f"refused {rc}: {capi.lib.dvbs2_last_error().decode()}"


def test_host_program_under_the_host_sanitizers(host_exe):
    inf, nan = np.inf, np.nan
    tiny, huge = float(np.float32(1e-45)), float(np.finfo(np.float32).max)  # the smallest denormal and the largest finite float32
    rows, want = [], []
    good = [(1e-5, 1.0, 1.0, 65536.0), (0.0, 0.0, 0.0, 0.0), (-0.0, -0.0, -0.0, -0.0), (tiny, tiny, tiny, tiny), (huge, huge, huge, huge),
            (0.0, -huge, -huge, 0.0), (1e-2, 1.0, -1.0, tiny)]
    bad = [(-tiny, 1.0, 1.0, 1.0), (-1.0, 1.0, 1.0, 1.0), (inf, 1.0, 1.0, 1.0), (-inf, 1.0, 1.0, 1.0), (nan, 1.0, 1.0, 1.0),
           (1e-5, inf, 1.0, 1.0), (1e-5, -inf, 1.0, 1.0), (1e-5, nan, 1.0, 1.0),
           (1e-5, 1.0, inf, 1.0), (1e-5, 1.0, -inf, 1.0), (1e-5, 1.0, nan, 1.0),
           (1e-5, 1.0, 1.0, -tiny), (1e-5, 1.0, 1.0, -1.0), (1e-5, 1.0, 1.0, inf), (1e-5, 1.0, 1.0, -inf), (1e-5, 1.0, 1.0, nan),
           (nan, nan, nan, nan)]
    for a in good:
        rows.append("check " + _hex(*a))
        want.append("ok")
        assert _lib_check(a) == "ok"
    for a in bad:
        rows.append("check " + _hex(*a))
        want.append(_lib_check(a))
        assert want[-1].startswith("refused -1: ")
    named = [w.split(": ")[1].split()[0] for w in want[len(good):]]
    assert named == ["rate"] * 5 + ["reference"] * 3 + ["gain"] * 3 + ["max_gain"] * 5 + ["rate"]  # the text names the argument
    # create: the parameter check first, then the corners of max_streams and max_samples
    ok = (1e-5, 1.0, 1.0, 65536.0)
    bad_creates = [((nan, 1.0, 1.0, 1.0), 1, 16), ((1e-5, 1.0, 1.0, -1.0), 1, 16), (ok, 0, 16), (ok, 65536, 16), (ok, -1, 16), (ok, 1, 0),
                   (ok, 1, (1 << 30) + 1), (ok, 1, -5)]
    for a, ms, mx in bad_creates:
        rows.append(f"create {_hex(*a)} {ms} {mx}")
        want.append(_lib_refuses_create(a, ms, mx))
    assert "max_streams" in want[-4] and "max_samples" in want[-1]
    rows.append("null")
    entries = ["reset", "set_params", "set_swap_iq", "set_gain", "params", "state", "work_device", "work"]
    want += [f"{e} -1: null handle" for e in entries] + ["create -1: null handle pointer", "destroy nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(want)
    for got, w in zip(lines, want):
        assert got == w
    assert sum(w.startswith("refused") for w in want) == len(bad) + len(bad_creates)
