"""CPU: the host-only side of the batched PL stages -- the argument ranges of dvbs2_plsync_batch_check and of the two batch creates, the
checks of a search call (dvbs2_plsync_batch_check_search: a null first or n_syms, counts, rows that run into each other), the stride rule
of the strided front end (dvbs2_plframe_stride_check), each refusal with its code and text -- through the library and once more in a
stand-alone program built with the host sanitizers, whose answers must be the library's. That the entries are bound and exported as
declared and answer a null handle as every other entry does is held by the censuses of tests/test_oracle_kat.py and
tests/test_capi_null_handle.py."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import PlSyncBatch, capi, plsync_batch_check

# the translation units of the entries and what they bind
SOURCES = ("c_api_plsync_batch.hip", "plsync_batch_hip.hip", "c_api_plcoarse.hip", "plcoarse_hip.hip", "c_api_plframe.hip", "plframe_hip.hip",
           "plpayload_hip.hip", "pl_signal.cpp")
EINVAL, ESIZE, EDEVICE = capi.EINVAL, capi.ESIZE, capi.EDEVICE
MIN = 33282 + 90
SHORT = P.plsc_of(1, 1, 1)  # QPSK 1/4 short with pilots: PLFRAME 8370
LEN = M.pls_parse(SHORT)["plframe_len"]

# (plsc, unlock_thresh, max_streams, max_symbols, max_frames) -> None (accepted) or the refusal's text; all refusals are EINVAL
CHECK = [((-1, 3, 1, MIN, 1), None), ((127, 255, 1024, 1 << 20, 1 << 20), None), ((0, 1, 64, MIN, 16), None),
         ((-1, 3, 0, MIN, 16), "max_streams out of range (1..1024)"), ((-1, 3, 1025, MIN, 16), "max_streams out of range (1..1024)"),
         ((-1, 3, -1, MIN, 16), "max_streams out of range (1..1024)"),
         ((-1, 3, 4, MIN - 1, 16), "max_symbols must be at least 33282 + 90"), ((-1, 3, 4, 0, 16), "max_symbols must be at least 33282 + 90"),
         ((-2, 3, 4, MIN, 16), "plsc out of range (-1 = decode every header, 0..127)"), ((128, 3, 4, MIN, 16), "plsc out of range (-1 = decode every header, 0..127)"),
         ((-1, 0, 4, MIN, 16), "unlock_thresh out of range (1..255)"), ((-1, 256, 4, MIN, 16), "unlock_thresh out of range (1..255)"),
         ((-1, 3, 4, MIN, 0), "max_frames out of range (1..1048576)"), ((-1, 3, 4, MIN, (1 << 20) + 1), "max_frames out of range (1..1048576)")]
# (period, plsc, max_streams, max_slots) of dvbs2_plcoarse_batch_create
COARSE = [((1, -1, 1, 1), None), ((7, 127, 1024, 1 << 20), None),
          ((0, -1, 4, 16), "period must be at least 1"), ((1, -2, 4, 16), "plsc out of range (-1 = not known, 0..127)"),
          ((1, 128, 4, 16), "plsc out of range (-1 = not known, 0..127)"), ((1, -1, 0, 16), "max_streams out of range (1..1024)"),
          ((1, -1, 1025, 16), "max_streams out of range (1..1024)"), ((1, -1, 4, 0), "max_slots out of range (1..1048576)"),
          ((1, -1, 4, (1 << 20) + 1), "max_slots out of range (1..1048576)")]
# (max_streams, max_symbols, stride, first or None, n_syms or None[, n_streams]) -> (code, text) or None
SEARCH = [((4, MIN, 40000, [0, 0], [MIN, 0]), None), ((4, MIN, 0, [], []), None), ((1, MIN, 0, [12345], [MIN]), None),
          ((4, MIN, 100, [1, 90], [99, 10]), None), ((4, MIN, 100, None, None, 0), None),
          ((4, MIN, 40000, None, [5, 5]), (EINVAL, "first is null")), ((4, MIN, 40000, [0, 0], None), (EINVAL, "n_syms is null")),
          ((4, MIN, 40000, None, None, 2), (EINVAL, "first is null")),
          ((1, MIN, 40000, [0, 0], [5, 5]), (ESIZE, "n_streams exceeds max_streams")), ((4, MIN, 40000, None, None, -1), (EINVAL, "n_streams is negative")),
          ((4, MIN, -1, [0, 0], [5, 5]), (EINVAL, "stride_syms is negative")),
          ((4, MIN, 40000, [0, -1], [5, 5]), (EINVAL, "first[1] is negative")), ((4, MIN, 40000, [0, 0], [5, -5]), (EINVAL, "n_syms[1] is negative")),
          ((4, MIN, 40000, [0, 0], [MIN + 1, 5]), (ESIZE, "n_syms[0] exceeds max_symbols")),
          ((4, MIN, 100, [1, 91], [99, 10]), (EINVAL, "first[1] + n_syms[1] exceeds stride_syms")),
          ((4, MIN, 100, [2, 0], [99, 10]), (EINVAL, "first[0] + n_syms[0] exceeds stride_syms"))]
STRIDE = [((SHORT, LEN + 90), None), ((SHORT, LEN + 91), None), ((SHORT, (1 << 31) - 1), None), ((0, 3330 + 90), None),
          ((SHORT, LEN + 89), (EINVAL, "stride_syms below plframe_len + 90")), ((SHORT, LEN), (EINVAL, "stride_syms below plframe_len + 90")),
          ((SHORT, 0), (EINVAL, "stride_syms below plframe_len + 90")), ((SHORT, -5), (EINVAL, "stride_syms below plframe_len + 90")),
          ((0, 3330 + 89), (EINVAL, "stride_syms below plframe_len + 90")), ((SHORT, 1 << 31), (EINVAL, "stride_syms above 2^31 - 1")),
          ((128, 40000), (EINVAL, "plsc out of range (0..127)")), ((-1, 40000), (EINVAL, "plsc out of range (0..127)"))]


def _said(code, want):
    text = capi.lib.dvbs2_last_error().decode()
    if want is None:
        assert code == capi.OK, text
        return "ok"
    assert (code, text) == want, (code, text, want)
    return f"refused {code}: {text}"


def _search_args(case):
    ms, mn, stride, first, n = case[:5]
    k = case[5] if len(case) > 5 else len(first if first is not None else n)
    return ms, mn, stride, first, n, k


def test_the_library_refuses_with_code_and_text():
    lib, h = capi.lib, C.c_void_p()
    for args, text in CHECK:
        _said(lib.dvbs2_plsync_batch_check(*args), text and (EINVAL, text))
        if text:
            with pytest.raises(capi.Dvbs2Error) as e:
                plsync_batch_check(*args)
            assert e.value.code == EINVAL and text in str(e.value)
            with pytest.raises(capi.Dvbs2Error):
                PlSyncBatch(args[0], args[1], args[2], args[3], args[4])  # refused before a device is looked for
            h.value = 1
            assert lib.dvbs2_plsync_batch_create(C.byref(h), *args, 0) == EINVAL and not h.value and lib.dvbs2_last_error().decode() == text
        else:
            plsync_batch_check(*args)
    for args, text in COARSE:
        if text:
            h.value = 1
            assert lib.dvbs2_plcoarse_batch_create(C.byref(h), *args, 0) == EINVAL and not h.value and lib.dvbs2_last_error().decode() == text
    for case, want in SEARCH:
        ms, mn, stride, first, n, k = _search_args(case)
        f = None if first is None else np.array(first + [0], np.int32)  # (one more, so that an empty list still has an address)
        c = None if n is None else np.array(n + [0], np.int32)
        _said(lib.dvbs2_plsync_batch_check_search(ms, mn, stride, f.ctypes.data if f is not None else None, c.ctypes.data if c is not None else None, k), want)
    for args, want in STRIDE:
        _said(lib.dvbs2_plframe_stride_check(*args), want)
    assert sum(t is not None for _, t in CHECK + COARSE + SEARCH + STRIDE) == 11 + 7 + 11 + 8


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/plsync_batch_host_main.cpp with the sources behind the entries, host code under AddressSanitizer and UBSan (device code is
    not instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("plsync_batch"), "plsync_batch_host_main.cpp", SOURCES)


NULL_ENTRIES = ("batch_reset", "batch_reset_stream", "batch_set_plsc_mode", "batch_set_expected_pls", "batch_search_device", "batch_finish",
                "batch_gather_device", "estimate_strided_device", "process_strided_device", "coarse_batch_reset", "coarse_batch_reset_stream",
                "coarse_batch_estimate_device")


def test_host_program_under_the_host_sanitizers(host_exe):
    rows, want = [], []

    def line(text, code=EINVAL):
        return "ok" if text is None else f"refused {code}: {text}"

    for args, text in CHECK:
        rows.append("check " + " ".join(map(str, args)))
        want.append(line(text))
        rows.append("create " + " ".join(map(str, args)))  # good arguments: refused where the device is looked for
        want.append(line(text) if text else line("this program looks for no device", EDEVICE))
    for args, text in COARSE:
        rows.append("coarse " + " ".join(map(str, args)))
        want.append(line(text) if text else line("this program looks for no device", EDEVICE))
    for case, w in SEARCH:
        ms, mn, stride, first, n, k = _search_args(case)
        k_vals = max(k, 0)
        vals = (first if first is not None else [0] * k_vals) + (n if n is not None else [0] * k_vals)
        rows.append(f"search {ms} {mn} {stride} {k} {int(first is not None)} {int(n is not None)} " + " ".join(map(str, vals)))
        want.append("ok" if w is None else line(w[1], w[0]))
    for args, w in STRIDE:
        rows.append("stride " + " ".join(map(str, args)))
        want.append("ok" if w is None else line(w[1], w[0]))
    rows.append("null")
    null_lines = [f"{e} {EINVAL}: null handle" for e in NULL_ENTRIES]
    null_lines += [f"batch_create {EINVAL}: null handle pointer", f"coarse_batch_create {EINVAL}: null handle pointer", "destroy nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(rows) - 1 + len(null_lines)
    for row, got, w in zip(rows[:-1], lines, want):
        assert got == w, (row[:80], got[:100], w[:100])
    assert lines[len(rows) - 1:] == null_lines
