"""CPU: the host side of the rotator rows' C ABI -- state_init, state_read, adjust_turns, rows_check and the argument checks of the three
device entries, which refuse before a device is looked for -- in a stand-alone program built with the host sanitizers
(tests/rotator_rows_host_main.cpp). Its answers must be the library's own, and both must be the model's (tests/rotator_rows_model.py):
adjust_turns the Python-int conversion exactly, state_init the extended-precision conversion of csrc/rotator_turns.h restated with
fractions. Nothing is loaded into Python by the program and no GPU call is made."""
import ctypes as C
import math

import numpy as np
import pytest

import fec_testlib as T
import rotator_rows_model as RM
from dvbs2rx_amd import ROTATOR_STATE, capi, rotator_adjust_turns, rotator_state_init, rotator_state_read

SOURCES = ("c_api_rotator_rows.hip", "rotator_rows_hip.hip")  # the entries' translation unit and what it binds
lib = capi.lib


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return T.build_host_program(tmp_path_factory.mktemp("rotator_rows"), "rotator_rows_host_main.cpp", SOURCES)


def f32(v):
    return "%08x" % np.array([v], np.float32).view(np.uint32)[0]


def f64(v):
    return "%016x" % np.array([v], np.float64).view(np.uint64)[0]


def said(rc):
    return "ok" if rc == capi.OK else f"refused {rc}: {lib.dvbs2_last_error().decode()}"


ESTIMATES = [0.0, -0.0, float(np.float32(1e-45)), 3.3875e-4, -3.3875e-4, 0.5, -0.5, np.nan, np.inf, -np.inf]
SCALES = [1.0, 0.5, 0.25, 1e-3, 0.0, 2.0, 1.0 / 3.0]
INCREMENTS = [0.0, math.pi, -math.pi, 2 * math.pi, 1e-300, 1e6]

# addresses that are never dereferenced: 16-byte aligned ones, one at +8, one at +4, one at +2
A, B8, C4, D2 = 0x10000, 0x20008, 0x30004, 0x40002
GOOD_ROWS = (A, 100, 0x50000, 100, 100, 2, 0, 0x60000)
GOOD_CONTROL = (A, 6, 12, 0x11000, 0x12000, 0x13000, 0x14000, 0x15000, 0.5, 0.5, 0, 0x60000, 0x16000, 0x17000)


def with_(args, **changes):
    names = changes.pop("_names")
    a = list(args)
    for k, v in changes.items():
        a[names.index(k)] = v
    return tuple(a)


ROWS_NAMES = ("d_in", "in_stride", "d_out", "out_stride", "n_samples", "n_streams", "base_index", "d_state")
CONTROL_NAMES = ("d_offsets", "n_streams", "max_slots", "cf", "cc", "ne", "ff", "fv", "coarse_scale", "fine_scale", "at_index", "d_state", "d_applied", "d_delta")
ROWS_REFUSED = [  # (changes, text)
    (dict(n_streams=0), "n_streams out of range (1..65535)"), (dict(n_streams=65536), "n_streams out of range (1..65535)"),
    (dict(n_samples=-1), "n_samples out of range (0..2^30)"), (dict(n_samples=(1 << 30) + 1, in_stride=1 << 31, out_stride=1 << 31), "n_samples out of range (0..2^30)"),
    (dict(in_stride=99), "in_stride is below n_samples"), (dict(out_stride=99), "out_stride is below n_samples"),
    (dict(base_index=-1), "base_index is negative"), (dict(base_index=(1 << 63) - 100), "base_index + n_samples overflows"),
    (dict(d_in=0), "in is null"), (dict(d_out=0), "out is null"), (dict(d_in=C4), "in and out must be 8-byte aligned"),
    (dict(d_out=C4), "in and out must be 8-byte aligned"), (dict(d_out=A, out_stride=101), "in place needs equal strides"),
    (dict(d_state=0), "state is null"), (dict(d_state=B8), "state must be 16-byte aligned")]
RETUNE_REFUSED = [((0, 0, 0, 0.1), "state is null"), ((B8, 0, 0, 0.1), "state must be 16-byte aligned"),
                  ((A, -1, 0, 0.1), "stream_index out of range (0..65534)"), ((A, 65535, 0, 0.1), "stream_index out of range (0..65534)"),
                  ((A, 0, -1, 0.1), "at_index is negative"), ((A, 0, 0, np.nan), "phase_inc must be finite"), ((A, 0, 0, np.inf), "phase_inc must be finite")]
CONTROL_REFUSED = [
    (dict(n_streams=0), "n_streams out of range (1..65535)"), (dict(n_streams=65536), "n_streams out of range (1..65535)"),
    (dict(max_slots=-1), "max_slots is negative"), (dict(d_offsets=0), "offsets is null"), (dict(cf=0), "coarse_foffset is null"),
    (dict(cc=0), "coarse_corrected is null"), (dict(ne=0), "new_est is null"), (dict(ff=0), "fine_foffset and fine_valid go together"),
    (dict(fv=0), "fine_foffset and fine_valid go together"), (dict(cc=D2), "the per-slot and per-stream arrays must be 4-byte aligned"),
    (dict(d_applied=D2), "the per-slot and per-stream arrays must be 4-byte aligned"), (dict(d_delta=C4), "delta must be 8-byte aligned"),
    (dict(coarse_scale=np.nan), "coarse_scale must be finite"), (dict(fine_scale=-np.inf), "fine_scale must be finite"),
    (dict(at_index=-1), "at_index is negative"), (dict(d_state=0), "state is null"), (dict(d_state=B8), "state must be 16-byte aligned")]


def rows_line(a):
    return "rows %x %d %x %d %d %d %d %x" % a


def retune_line(a):
    return "retune %x %d %d %s" % (a[0], a[1], a[2], f64(a[3]))


def control_line(a):
    return "control %x %d %d %x %x %x %x %x %s %s %d %x %x %x" % (*a[:8], f64(a[8]), f64(a[9]), *a[10:])


def test_adjust_turns_is_the_python_int_conversion():
    """every estimate with every scale: delta is rint(float64(float32(e)) * scale * 2^64) exactly, applies is false exactly for a product
    that is not finite or not below a half"""
    n_false = 0
    for e in ESTIMATES:
        for scale in SCALES:
            with np.errstate(invalid="ignore"):
                d = np.float64(np.float32(e)) * np.float64(scale)
            want_applies = bool(np.isfinite(d) and abs(d) < 0.5)
            delta, applies = rotator_adjust_turns(e, scale)
            assert applies == want_applies == RM.adjust_turns(e, scale)[1], (e, scale)
            if applies:
                assert delta == int(np.rint(np.float64(np.float32(e)) * scale * 2.0 ** 64)) == RM.adjust_turns(e, scale)[0], (e, scale)
            else:
                assert delta == 0
                n_false += 1
    # 0.5 and -0.5 with the scales 1 and 2; NaN with all seven; +-inf with all seven (inf * 0 is NaN)
    assert n_false == 4 + 7 + 14
    assert rotator_adjust_turns(3.3875e-4, 0.5)[0] == int(np.rint(float(np.float32(3.3875e-4)) * 0.5 * 2.0 ** 64))


def test_state_init_is_the_conversion_of_the_single_rotator():
    """the records' inc equals rotator_inc_turns restated with fractions, operation by operation; the exact quotient (plcoarse_model.turns,
    160 fraction bits) is within the conversion's stated 2^-63 relative + half a unit of it"""
    st = rotator_state_init(INCREMENTS)
    assert st.dtype == ROTATOR_STATE and ROTATOR_STATE.itemsize == 32
    assert not st["phase"].any() and not st["index"].any() and not st["reserved"].any()
    for inc, r in zip(INCREMENTS, st):
        assert int(r["inc"]) == RM.inc_turns(inc), inc
        exact = RM.R.turns(inc) / 2.0 ** (RM.R.FRAC - 64)
        err = (int(r["inc"]) - exact + 2.0 ** 63) % 2.0 ** 64 - 2.0 ** 63
        # in units of 2^-64 turns: the quotient's two roundings (2^-63 relative to |inc| / 2 pi), the floor's difference (2^-65 turns)
        # and the final rounding (half a unit)
        assert abs(err) <= 1.0 + 2.0 * abs(inc) / (2 * math.pi), (inc, err)
    inc, phase = rotator_state_read(st)
    # (the double nearest to pi is 1.2e-16 below pi: some 360 units of 2^-64 turns, so these are near and not equal)
    assert np.allclose(inc[:5], [0.0, math.pi, -math.pi, 0.0, 0.0], rtol=0, atol=1e-15) and not phase.any()
    assert (np.abs(inc) <= math.pi).all()
    back = rotator_state_read(np.array([((1 << 63) + 1, (1 << 64) - 1, 7, 9), (1 << 62, 3 << 62, -4, 0), (1 << 63, 1 << 63, 0, 0)], ROTATOR_STATE))
    assert back[0].tolist() == [-2.0 ** -64 * 2 * math.pi, -math.pi / 2, math.pi] and back[1][1:].tolist() == [math.pi / 2, math.pi]
    assert -math.pi <= back[1][0] < -3.14159


def test_host_program_under_the_host_sanitizers(host_exe):
    rows, want = [], []
    # state_init: the increments one by one and together; a value that is not finite is named and nothing is written
    for incs in [[v] for v in INCREMENTS] + [INCREMENTS]:
        rows.append("init %d %s" % (len(incs), " ".join(f64(v) for v in incs)))
        want.append("ok " + " ".join("%x" % RM.inc_turns(v) for v in incs))
        assert ["%x" % int(v) for v in rotator_state_init(incs)["inc"]] == want[-1].split()[1:]
    for incs, where in (([0.1, np.nan, 0.2], 1), ([np.inf], 0), ([0.1, 0.2, 0.3, -np.inf], 3)):
        rows.append("init %d %s" % (len(incs), " ".join(f64(v) for v in incs)))
        a, st = np.array(incs), np.zeros(len(incs), ROTATOR_STATE)
        T.refused(capi.EINVAL, f"phase_inc[{where}] must be finite", lib.dvbs2_rotator_state_init, a.ctypes.data, len(incs), st.ctypes.data)
        assert not st.view(np.uint64).any()
        want.append(f"refused -1: phase_inc[{where}] must be finite untouched")
    # state_read
    for phase, inc in ((0, 0), (1 << 63, 1 << 63), ((1 << 63) + 1, (1 << 64) - 1), (1 << 62, 3 << 62), (12345, 0xfedcba9876543210)):
        rows.append("read %x %x" % (phase, inc))
        got = rotator_state_read(np.array([(phase, inc, 5, 9)], ROTATOR_STATE))
        # (-pi, pi]: the double -math.pi lies INSIDE, it is 1.2e-16 above -pi, and is what turns a unit above a half come back as
        assert -math.pi <= got[0][0] <= math.pi and -math.pi <= got[1][0] <= math.pi
        want.append("ok %s %s" % (f64(got[0][0]).lstrip("0") or "0", f64(got[1][0]).lstrip("0") or "0"))
    # adjust_turns
    for e in ESTIMATES:
        for scale in SCALES:
            rows.append(f"adjust {f32(e)} {f64(scale)}")
            delta, applies = RM.adjust_turns(e, scale)
            want.append(f"ok {delta} {int(applies)}")
    # rows_check: the corners of every range
    checks = [((5, 5, 5, 1, 0), None), ((0, 0, 5, 1, 0), None), ((5, 5, 0, 2, 0), None), ((1 << 30, 1 << 30, 1 << 30, 65535, 0), None),
              ((5, 5, 5, 2, (1 << 63) - 6), None), ((5, 5, 5, 0, 0), "n_streams"), ((5, 5, 5, 65536, 0), "n_streams"), ((5, 5, -1, 1, 0), "n_samples"),
              ((1 << 31, 1 << 31, (1 << 30) + 1, 1, 0), "n_samples"), ((4, 5, 5, 2, 0), "in_stride"), ((5, 4, 5, 2, 0), "out_stride"),
              ((5, 5, 5, 1, -1), "base_index"), ((5, 5, 5, 1, (1 << 63) - 5), "base_index")]
    for a, named in checks:
        rows.append("check %d %d %d %d %d" % a)
        want.append(said(lib.dvbs2_rotator_rows_check(*a)))
        assert want[-1] == "ok" if named is None else want[-1].startswith(f"refused -1: {named} "), (a, want[-1])
    # the device entries: every refusal with its exact text, from the program and from the library; arguments that pass every check reach
    # the device lookup, which this program answers itself
    no_device = "refused -2: this program looks for no device"
    rows.append(rows_line(GOOD_ROWS))
    want.append(no_device)
    rows.append(rows_line(with_(GOOD_ROWS, _names=ROWS_NAMES, n_samples=0, d_in=0, d_out=0, d_state=0)))  # nothing to do: no pointer is looked at
    want.append("ok")
    assert lib.dvbs2_rotator_rows_device(None, 100, None, 100, 0, 2, 0, None, 0, None) == capi.OK
    for changes, text in ROWS_REFUSED:
        a = with_(GOOD_ROWS, _names=ROWS_NAMES, **changes)
        rows.append(rows_line(a))
        want.append(f"refused -1: {text}")
        T.refused(capi.EINVAL, text, lib.dvbs2_rotator_rows_device, *[v or None if i in (0, 2, 7) else v for i, v in enumerate(a)], 0, None)
    rows.append(retune_line((A, 65534, 1 << 62, -0.1)))
    want.append(no_device)
    for a, text in RETUNE_REFUSED:
        rows.append(retune_line(a))
        want.append(f"refused -1: {text}")
        T.refused(capi.EINVAL, text, lib.dvbs2_rotator_retune_device, a[0] or None, a[1], a[2], float(a[3]), 0, None)
    for good in (GOOD_CONTROL, with_(GOOD_CONTROL, _names=CONTROL_NAMES, ff=0, fv=0, d_applied=0, d_delta=0, max_slots=0)):
        rows.append(control_line(good))
        want.append(no_device)
    for changes, text in CONTROL_REFUSED:
        a = with_(GOOD_CONTROL, _names=CONTROL_NAMES, **changes)
        rows.append(control_line(a))
        want.append(f"refused -1: {text}")
        T.refused(capi.EINVAL, text, lib.dvbs2_rotator_control_device, *[v or None if i in (0, 3, 4, 5, 6, 7, 11, 12, 13) else v for i, v in enumerate(a)], 0, None)
    rows.append("null")
    want += ["init-inc -1: phase_inc is null", "init-state -1: state is null", "init-count -1: n_streams out of range (1..65535)",
             "read-state -1: state is null", "read-count -1: n_streams out of range (1..65535)", "adjust-delta -1: delta is null",
             "adjust-applies -1: applies is null", "outputs nothing written"]
    lines = T.run_host_program(host_exe, rows)
    assert len(lines) == len(want)
    for row, got, w in zip(rows + ["null"] * 7, lines, want):
        assert got == w, row
