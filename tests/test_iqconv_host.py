"""CPU: the host-only side of the IQ sample converter's C ABI -- dvbs2_iqconv_check at the corners of every refusal, the argument checks of
create, blocks of the host restatement across an odd length and an odd byte offset, and every new entry with a null handle -- once more
in a stand-alone program built with the host sanitizers. Its answers must be the library's own. Nothing is loaded into Python by the
program and no GPU call is made."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
import iqconv_model as M
from dvbs2rx_amd import capi

SOURCES = ("c_api_iqconv.hip", "iqconv_hip.hip")  # the entries' translation unit and what it binds


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/iqconv_host_main.cpp with the sources behind the entries, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("iqconv"), "iqconv_host_main.cpp", SOURCES)


def _hex(value):
    return "%08x" % int(np.array(value, np.float32).view(np.uint32))


def _lib_check(fmt, gain, max_streams, max_samples):
    rc = capi.lib.dvbs2_iqconv_check(fmt, float(np.float32(gain)), max_streams, max_samples)
    return "ok" if rc == capi.OK else f"refused {rc}: {capi.lib.dvbs2_last_error().decode()}"


def _lib_refuses_create(fmt, gain, max_streams, max_samples):
    h = C.c_void_p()
    rc = capi.lib.dvbs2_iqconv_create(C.byref(h), fmt, float(np.float32(gain)), max_streams, max_samples, 0)
    assert rc == capi.EINVAL and not h  # every row below is refused before a device is looked for
    return f"refused {rc}: {capi.lib.dvbs2_last_error().decode()}"


def test_host_program_under_the_host_sanitizers(host_exe):
    inf, nan = np.inf, np.nan
    lo, hi = np.float32(2.0 ** -64), np.float32(2.0 ** 64)
    under, over = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(inf))
    rows, want = [], []
    for fmt in (-1, 0, 1, 2, 3):
        rows.append(f"bytes {fmt}")
        want.append(str(capi.lib.dvbs2_iqconv_bytes(fmt)))
    assert want == ["-1", "2", "2", "4", "-1"]
    good = [(0, 1.0, 1, 1), (1, lo, 65535, 1 << 30), (2, hi, 1, 1), (2, 0.3, 65535, 1), (0, 16.0, 1, 1 << 30)]
    bad = [(-1, 1.0, 1, 1), (3, 1.0, 1, 1),
           (0, 0.0, 1, 1), (0, -0.0, 1, 1), (0, -1.0, 1, 1), (1, inf, 1, 1), (1, -inf, 1, 1), (2, nan, 1, 1), (2, under, 1, 1), (0, over, 1, 1),
           (0, np.float32(1e-45), 1, 1),
           (0, 1.0, 0, 1), (0, 1.0, -1, 1), (0, 1.0, 65536, 1), (0, 1.0, 1, 0), (0, 1.0, 1, -1), (0, 1.0, 1, (1 << 30) + 1), (3, nan, 0, 0)]
    for a in good:
        rows.append(f"check {a[0]} {_hex(a[1])} {a[2]} {a[3]}")
        want.append("ok")
        assert _lib_check(*a) == "ok"
    for a in bad:
        rows.append(f"check {a[0]} {_hex(a[1])} {a[2]} {a[3]}")
        want.append(_lib_check(*a))
        assert want[-1].startswith("refused -1: ")
    named = [w.split(": ")[1].split()[0] for w in want[-len(bad):]]
    assert named == ["format"] * 2 + ["gain"] * 9 + ["max_streams"] * 3 + ["max_samples"] * 3 + ["format"]  # the text names the argument
    bad_creates = [(3, 1.0, 1, 16), (-1, 1.0, 1, 16), (0, nan, 1, 16), (0, 0.0, 1, 16), (1, under, 1, 16), (2, over, 1, 16), (0, 1.0, 0, 16),
                   (0, 1.0, 65536, 16), (0, 1.0, 1, 0), (0, 1.0, 1, (1 << 30) + 1)]
    for a in bad_creates:
        rows.append(f"create {a[0]} {_hex(a[1])} {a[2]} {a[3]}")
        want.append(_lib_refuses_create(*a))
    assert "format" in want[-10] and "gain" in want[-5] and "max_streams" in want[-3] and "max_samples" in want[-1]
    # blocks of the host restatement, an odd number of samples at an odd byte offset (s16: an even one that is no multiple of 4): the
    # program's own compilation of iqconv_math.hpp against the library's, which tests/test_iqconv_model.py holds to the model
    rng = np.random.default_rng(7)
    n = 37
    for fmt in M.FORMATS:
        for offset in (0, 3, 2) if fmt != M.S16 else (0, 2, 6):
            gain = np.float32(0.3 if offset else 1.0)
            codes = rng.integers(M.LO[fmt], M.HI[fmt] + 1, (1, n, 2)).astype(M.DTYPE[fmt])
            codes[0, 0, 0], codes[0, n - 1, 1] = M.LO[fmt], M.HI[fmt]
            y, st = M.unpack_rows(fmt, gain, codes)
            rows.append(f"unpack {fmt} {_hex(gain)} {offset} {n} " + " ".join(str(int(c)) for c in codes.reshape(-1)))
            want.append(" ".join("%08x" % b for b in y.reshape(-1).view(np.uint32)) + " | %d %d %d" % tuple(st[0]))
            x = np.resize(np.concatenate([M.edge_values(fmt), (rng.normal(size=16) * 0.7).astype(np.float32)]), 2 * n).reshape(1, n, 2)
            c, st = M.pack_rows(fmt, gain, x)
            rows.append(f"pack {fmt} {_hex(gain)} {offset} {n} " + " ".join(_hex(v) for v in x.reshape(-1)))
            want.append(" ".join(str(int(v)) for v in c.reshape(-1)) + " | %d %d %d" % tuple(st[0]))
    rows.append("null")
    entries = ["set_gain", "params", "unpack_device", "pack_device", "unpack_to_device", "pack_from_device"]
    want += [f"{e} -1: null handle" for e in entries] + ["create -1: null handle pointer", "destroy nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(want)
    for got, w_ in zip(lines, want):
        assert got == w_
    assert sum(w_.startswith("refused") for w_ in want) == len(bad) + len(bad_creates)
