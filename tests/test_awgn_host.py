"""CPU: the host-only side of the AWGN channel's C ABI -- dvbs2_awgn_check at the corners of every refusal, the argument checks of
create, a block of the host restatement, and every new entry with a null handle -- once more in a stand-alone program built with the
host sanitizers. Its answers must be the library's own. Nothing is loaded into Python by the program and no GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
from dvbs2rx_amd import capi

SOURCES = ("c_api_channel.hip", "awgn_hip.hip")  # the entries' translation unit and what it binds
SEED, STREAM, FIRST, COUNT = 0xC0FFEE0123456789, (1 << 64) - 3, (1 << 33) - 37, 96  # a block across the counter's carry


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/awgn_host_main.cpp with the sources behind the entries, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("awgn"), "awgn_host_main.cpp", SOURCES)


def _hex(value):
    return "%08x" % int(np.array(value, np.float32).view(np.uint32))


def _lib_check(sigma, max_streams, max_samples):
    rc = capi.lib.dvbs2_awgn_check(float(np.float32(sigma)), max_streams, max_samples)
    return "ok" if rc == capi.OK else f"refused {rc}: {capi.lib.dvbs2_last_error().decode()}"


def _lib_refuses_create(sigma, max_streams, max_samples):
    h = C.c_void_p()
    rc = capi.lib.dvbs2_awgn_create(C.byref(h), 1, float(np.float32(sigma)), max_streams, max_samples, 0)
    assert rc == capi.EINVAL and not h  # every row below is refused before a device is looked for
    return f"refused {rc}: {capi.lib.dvbs2_last_error().decode()}"


def test_host_program_under_the_host_sanitizers(host_exe):
    inf, nan = np.inf, np.nan
    tiny, huge = float(np.float32(1e-45)), float(np.finfo(np.float32).max)  # the smallest denormal and the largest finite float32
    rows, want = [], []
    good = [(0.0, 1, 1), (-0.0, 1, 1), (tiny, 65535, 1 << 30), (huge, 1, 1), (1.0, 65535, 1), (1.0, 1, 1 << 30)]
    bad = [(-tiny, 1, 1), (-1.0, 1, 1), (inf, 1, 1), (-inf, 1, 1), (nan, 1, 1),
           (1.0, 0, 1), (1.0, -1, 1), (1.0, 65536, 1), (1.0, 1, 0), (1.0, 1, -1), (1.0, 1, (1 << 30) + 1), (nan, 0, 0)]
    for a in good:
        rows.append(f"check {_hex(a[0])} {a[1]} {a[2]}")
        want.append("ok")
        assert _lib_check(*a) == "ok"
    for a in bad:
        rows.append(f"check {_hex(a[0])} {a[1]} {a[2]}")
        want.append(_lib_check(*a))
        assert want[-1].startswith("refused -1: ")
    named = [w.split(": ")[1].split()[0] for w in want[len(good):]]
    assert named == ["sigma"] * 5 + ["max_streams"] * 3 + ["max_samples"] * 3 + ["sigma"]  # the text names the argument
    bad_creates = [(nan, 1, 16), (-1.0, 1, 16), (inf, 1, 16), (1.0, 0, 16), (1.0, 65536, 16), (1.0, -1, 16), (1.0, 1, 0), (1.0, 1, (1 << 30) + 1),
                   (1.0, 1, -5)]
    for a in bad_creates:
        rows.append(f"create {_hex(a[0])} {a[1]} {a[2]}")
        want.append(_lib_refuses_create(*a))
    assert "max_streams" in want[-4] and "max_samples" in want[-1]
    # a block of the host restatement: the program's own compilation of awgn_math.hpp against the library's
    rows.append(f"sample {SEED} {STREAM} {FIRST} {COUNT}")
    w, v = np.zeros(2, np.uint32), np.zeros(2, np.float32)
    for i in range(COUNT):
        assert capi.lib.dvbs2_awgn_words(SEED, STREAM, FIRST + i, w.ctypes.data) == capi.OK
        assert capi.lib.dvbs2_awgn_sample(SEED, STREAM, FIRST + i, v.ctypes.data) == capi.OK
        want.append("%08x %08x %08x %08x" % (w[0], w[1], *v.view(np.uint32)))
    rows.append("null")
    entries = ["set_sigma", "set_seed", "params", "add_device", "add"]
    want += [f"{e} -1: null handle" for e in entries] + ["create -1: null handle pointer", "destroy nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(want)
    for got, w_ in zip(lines, want):
        assert got == w_
    assert sum(w_.startswith("refused") for w_ in want) == len(bad) + len(bad_creates)
