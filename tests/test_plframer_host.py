"""CPU: the host side of the PL framer -- dvbs2_plframer_layout over the whole PLSC range and a named sequence, and the layout code once more in a stand-alone program built with the host sanitizers."""
import subprocess

import numpy as np
import pytest

import fec_testlib as T
import plframe_model as M
import plframer_model as F
import plsync_model as PS
from dvbs2rx_amd import capi, plframer_layout, pls_parse


def _err():
    return capi.lib.dvbs2_last_error().decode()


def _layout_rc(plscs):
    a = np.ascontiguousarray(plscs, np.uint8)
    return capi.lib.dvbs2_plframer_layout(a.ctypes.data, int(a.size), None, None, None, None)


def test_layout_over_the_whole_plsc_range():
    for plsc in range(128):
        if plsc >> 2 in F.RESERVED:
            assert _layout_rc([plsc]) == capi.EINVAL and _err() == "plsc[0] names a reserved MODCOD (29..31)", plsc
            assert _layout_rc([4, 4, plsc]) == capi.EINVAL and _err() == "plsc[2] names a reserved MODCOD (29..31)", plsc
            continue
        lay, p = plframer_layout([plsc]), pls_parse(plsc)
        assert lay["in_offset"].tolist() == [0] and lay["out_offset"].tolist() == [0]
        assert lay["out_syms"] == p["plframe_len"] == M.pls_parse(plsc)["plframe_len"]
        assert lay["in_syms"] == (0 if plsc >> 2 == 0 else p["xfecframe_len"])
    assert _layout_rc([128]) == capi.EINVAL and _err() == "plsc[0] out of range (0..127)"
    assert _layout_rc([4, 255]) == capi.EINVAL and _err() == "plsc[1] out of range (0..127)"
    assert capi.lib.dvbs2_plframer_layout(None, 1, None, None, None, None) == capi.EINVAL
    empty = plframer_layout([])
    assert (empty["in_syms"], empty["out_syms"], empty["in_offset"].size) == (0, 0, 0)


def test_layout_of_the_named_sequence_is_the_running_sums():
    lay, want = plframer_layout(PS.ACM_PLSCS), F.layout(PS.ACM_PLSCS)
    infos = [M.pls_parse(p) for p in PS.ACM_PLSCS]
    run_in = np.concatenate([[0], np.cumsum([0 if i["dummy_frame"] else i["xfecframe_len"] for i in infos])])
    run_out = np.concatenate([[0], np.cumsum([i["plframe_len"] for i in infos])])
    assert lay["in_offset"].tolist() == run_in[:-1].tolist() == want["in_offset"].tolist()
    assert lay["out_offset"].tolist() == run_out[:-1].tolist() == want["out_offset"].tolist()
    assert (lay["in_syms"], lay["out_syms"]) == (run_in[-1], run_out[-1]) == (want["in_syms"], want["out_syms"])
    assert sum(i["dummy_frame"] for i in infos) == 2  # the sequence does hold frames that read nothing


@pytest.fixture(scope="module")
def layout_exe(tmp_path_factory):
    """tests/plframer_host_main.cpp with the host source it calls, host code under AddressSanitizer and UBSan (device code is not
    instrumented and none of it runs)."""
    return T.build_host_program(tmp_path_factory.mktemp("plframer"), "plframer_host_main.cpp", ("pl_signal.cpp",), fp_contract_off=False)


def test_layout_program_under_the_host_sanitizers(layout_exe):
    seqs = [[p] for p in range(129)] + [list(PS.ACM_PLSCS), PS.ACM_PLSCS[:5] + [29 << 2] + PS.ACM_PLSCS[5:], PS.ACM_PLSCS * 40, []]
    text = "".join(" ".join(map(str, s)) + "\n" for s in seqs)
    r = subprocess.run([layout_exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report goes to stderr and ends the program
    lines = r.stdout.splitlines()
    assert len(lines) == len(seqs)
    n_refused = 0
    for seq, line in zip(seqs, lines):
        bad = [i for i, p in enumerate(seq) if p > 127 or p >> 2 in F.RESERVED]
        if bad:
            why = "out of range (0..127)" if seq[bad[0]] > 127 else "names a reserved MODCOD (29..31)"
            assert line == "refused: plsc[%d] %s" % (bad[0], why), seq
            n_refused += 1
            continue
        want = F.layout(seq)
        offs, totals = line.split("|")
        assert [tuple(map(int, t.split(":"))) for t in offs.split()] == list(zip(want["in_offset"].tolist(), want["out_offset"].tolist())), seq
        assert tuple(map(int, totals.split())) == (want["in_syms"], want["out_syms"]), seq
    assert n_refused == 12 + 1 + 1
