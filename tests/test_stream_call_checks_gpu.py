"""The order of the call checks of every stream stage's work entries, and that a refused call leaves the handle as it was.

One handle per stage at its smallest legal size (AGC, AWGN, IQ converter: max_streams 2, max_samples 2; pulse shaper: sps 2, one tap;
resampler: nfilts 2, two taps, rate 1; down-converter: decim 1, one tap, two channels, two inputs; spectrum: nfft = hop = max_samples = 64).
Every work entry of the stage is given the same table of calls, each of which has TWO faults or none, so that the answer says which
check stands first:
  - count negative and rows above the cap     -> "<n> is negative", EINVAL
  - count above the cap and rows negative     -> "n_streams is negative", EINVAL
  - both above their caps                     -> "<n> exceeds <cap>", ESIZE
  - rows above the cap with null buffers      -> "n_streams exceeds max_streams", ESIZE
  - count 0 with null buffers, and with buffers of a sentinel -> OK, the buffers untouched, a reported count 0
  - both buffers null, then only `out`, then only `in` -> the entry's answer for each
  - both buffers misaligned by 4 bytes        -> the entry's alignment text
(a host-buffer entry of one row has no rows and no alignment cases; the down-converter's table carries its third count, the AWGN's a
negative first_index with a null `out`). Every case returns from the argument checks: nothing is launched, the buffers handed to a
refused call are host memory that must keep its sentinel. Behind the table one good call on the same handle must equal, byte for byte,
the call on a handle that never failed, and that must equal the stage's model (tests/*_model.py) bit for bit.
The codes and texts were recorded from the library before the stream entries shared their checks."""
import ctypes as C
import functools

import numpy as np
import pytest

import agc_model as AM
import awgn_model as WM
import ddc_model as DM
import fec_testlib as T
import iqconv_model as IQ
import pulse_model as PM
import resamp_model as RM
import spectrum_model as SM
from dvbs2rx_amd import Agc, Awgn, Ddc, IqConverter, PulseShaper, Resampler, Rotator, Spectrum, capi, spectrum_twiddles, spectrum_window
from dvbs2rx_amd.capi import lib

pytestmark = pytest.mark.gpu

EINVAL, ESIZE, OK = capi.EINVAL, capi.ESIZE, capi.OK
FILL = 0xA5
ROOM = np.full(1 << 12, FILL, np.uint8)  # what a refused call is given for a buffer: never read, never written
R = ROOM.ctypes.data + (-ROOM.ctypes.data) % 8
S = 64  # every stride: at least the largest count a case passes
SENT = -7  # in a host-side count before the call
ALIGN = "in and out must be 8-byte aligned"
IN0, OUT0 = "in is null", "out is null"


def cplx(key, n):
    rng = np.random.default_rng([91, key])
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)


def blob(*parts):
    return b"|".join(np.ascontiguousarray(a).tobytes() for a in parts)


# ------------------------------------------------------------------ per stage: the handle, the good call (bytes), the model's bytes
def agc_make():
    return Agc(0.05, 1.0, 1.0, 65536.0, max_streams=2, max_samples=2)


def agc_good(o):
    return blob(*o.work(cplx(1, 2)))


def agc_model():
    out, gains = AM.AgcModel(0.05, 1.0, 1.0, 65536.0, 2).work(cplx(1, 2))
    return blob(out[0], gains[0])


def awgn_make():
    return Awgn(seed=5, sigma=0.75, max_streams=2, max_samples=2)


def awgn_good(o):
    return blob(o.work(cplx(2, 2), stream_id=3, first_index=10))


def awgn_model():
    return blob(WM.rows(5, 3, 10, 2, 1, np.float32(0.75), cplx(2, 2).view(np.float32).reshape(1, 2, 2)).astype(np.float32))


IQ_CODES = np.array([[0, 255], [128, 37]], np.uint8)


def iqconv_make():
    return IqConverter("u8", 1.0, max_streams=2, max_samples=2)


def iqconv_good(o):
    import torch
    d = torch.zeros(4, dtype=torch.float32, device="cuda")
    o.unpack_to_device(IQ_CODES, d.data_ptr())
    return blob(d.cpu().numpy(), o.pack_from_device(d.data_ptr(), 2))


def iqconv_model():
    y = IQ.unpack(IQ.U8, 1.0, IQ_CODES)[0]
    return blob(y, IQ.pack(IQ.U8, 1.0, y)[0])


PULSE_TAPS = np.array([0.5], np.float32)


def pulse_make():
    return PulseShaper(sps=2, max_streams=2, max_symbols=2, taps=PULSE_TAPS)


def pulse_good(o):
    return blob(o.work(cplx(4, 2)))


def pulse_model():
    return blob(PM.shape32(PULSE_TAPS, 2, cplx(4, 2))[0])


RESAMP_TAPS = np.array([0.5, 0.25], np.float32)


def resamp_make():
    return Resampler(2, RESAMP_TAPS, 1.0, max_streams=2, max_samples=2)


def resamp_good(o):
    return blob(o.work(cplx(5, 2)))


def resamp_model():
    return blob(RM.resample32(RESAMP_TAPS, 2, cplx(5, 2), RM.step_of(1.0))[0])


DDC_TAPS = np.array([0.5], np.float32)
DDC_INCS = (0.1, -0.2)


def ddc_make():
    o = Ddc(1, DDC_TAPS, max_channels=2, max_inputs=2, max_samples=2)
    for c, inc in enumerate(DDC_INCS):
        o.set_channel(c, inc, input=c)
    return o


def ddc_good(o):
    return blob(o.work(cplx(6, 4).reshape(2, 2)))


def ddc_model():
    """model (a) of ddc_model.py over what the rotator stage gives on the device, as tests/test_ddc_gpu.py has it"""
    import torch
    x, outs = cplx(6, 4).reshape(2, 2), []
    for c, inc in enumerate(DDC_INCS):
        rot = Rotator(inc)
        d_x = torch.from_numpy(x[c].copy().view(np.float32)).cuda()
        d_z = torch.empty_like(d_x)
        rot.work_device(d_x.data_ptr(), 2, d_z.data_ptr(), T.stream())
        torch.cuda.synchronize()
        outs.append(DM.decimate32(DDC_TAPS, 1, d_z.cpu().numpy().view(np.complex64), 0, None)[0])
        rot.close()
    return blob(np.stack(outs))


def spectrum_make():
    return Spectrum(64, hop=64, avg=0, max_streams=2, max_samples=64)


def spectrum_good(o):
    return blob(o.work(cplx(7, 64)))


def spectrum_model():
    return blob(SM.rows32(cplx(7, 64), 64, 64, 0, spectrum_window("hann", 64), spectrum_twiddles(64), True))


STAGES = {"agc": (agc_make, agc_good, agc_model), "awgn": (awgn_make, awgn_good, awgn_model), "iqconv": (iqconv_make, iqconv_good, iqconv_model),
          "pulse": (pulse_make, pulse_good, pulse_model), "resamp": (resamp_make, resamp_good, resamp_model),
          "ddc": (ddc_make, ddc_good, ddc_model), "spectrum": (spectrum_make, spectrum_good, spectrum_model)}


@functools.lru_cache(None)
def reference(stage):
    """the good call on a handle that never failed; it is the model's answer bit for bit"""
    make, good, model = STAGES[stage]
    o = make()
    out = good(o)
    o.close()
    assert np.array_equal(np.frombuffer(out, np.uint8), np.frombuffer(model(), np.uint8)), f"{stage}: the device is not the model"
    return out


# ------------------------------------------------------------------ the entries
class Entry:
    """call(o, counts, a, b, said, **kw) -> code: counts is (n, rows) -- (n, n_inputs, n_channels) for the down-converter --, a and b
    the in and out buffers, said a c_int64 array for the host-side counts the entry reports. count / cap: the names in the entry's texts;
    top: the cap's value; one: a count at which the entry comes to its buffers; rows: it takes a row count; null: its answers to
    (both null, out null, in null), None where that is no refusal; align: its answer to buffers misaligned by 4 bytes, None where it
    has no such check; refused_says: what it leaves in its first host-side count when it refuses."""

    def __init__(self, stage, name, call, count, cap, top=2, one=1, rows=True, null=(IN0, OUT0, IN0), align=ALIGN, refused_says=SENT, extra=()):
        self.stage, self.name, self.call, self.count, self.cap, self.top, self.one, self.rows = stage, name, call, count, cap, top, one, rows
        self.null, self.align, self.refused_says, self.extra = null, align, refused_says, extra

    def table(self):
        """(what, counts, a, b, kw, code, text)"""
        n, cap, top, one = self.count, self.cap, self.top, self.one
        if self.stage == "ddc":
            yield from [("count negative, rows above", (-1, 3, 3), R, R, {}, EINVAL, "n_in is negative"),
                        ("count above, rows negative", (top + 1, -1, -1), R, R, {}, EINVAL, "n_inputs is negative"),
                        ("count and inputs above, channels negative", (top + 1, 3, -1), R, R, {}, EINVAL, "n_channels is negative"),
                        ("all above", (top + 1, 3, 3), R, R, {}, ESIZE, "n_in exceeds max_samples"),
                        ("inputs and channels above, null buffers", (one, 3, 3), None, None, {}, ESIZE, "n_inputs exceeds max_inputs"),
                        ("channels above, null buffers", (one, 1, 3), None, None, {}, ESIZE, "n_channels exceeds max_channels"),
                        ("a channel's input missing, null buffers", (one, 1, 2), None, None, {}, EINVAL, IN0),
                        ("a channel's input missing", (one, 1, 2), R, R, {}, EINVAL, "channel 1 reads input 1, which is not below n_inputs")]
            rows1 = (1, 1)
        elif self.rows:
            yield from [("count negative, rows above", (-1, 3), R, R, {}, EINVAL, f"{n} is negative"),
                        ("count above, rows negative", (top + 1, -1), R, R, {}, EINVAL, "n_streams is negative"),
                        ("both above", (top + 1, 3), R, R, {}, ESIZE, f"{n} exceeds {cap}"),
                        ("rows above, null buffers", (one, 3), None, None, {}, ESIZE, "n_streams exceeds max_streams")]
            rows1 = (1,)
        else:
            yield from [("count negative, null buffers", (-1, 1), None, None, {}, EINVAL, f"{n} is negative"),
                        ("count above, null buffers", (top + 1, 1), None, None, {}, ESIZE, f"{n} exceeds {cap}")]
            rows1 = (1,)
        yield ("count 0, null buffers", (0, *rows1), None, None, {}, OK, None)
        yield ("count 0", (0, *rows1), R, R, {}, OK, None)
        for what, a, b, text in zip(("both null", "out null", "in null"), (None, R, None), (None, None, R), self.null):
            if text is not None:
                yield (what, (one, *rows1), a, b, {}, EINVAL, text)
        if self.align is not None:
            yield ("misaligned by 4", (one, *rows1), R + 4, R + 4, {}, EINVAL, self.align)
        for what, counts, a, b, kw, code, text in self.extra:
            yield (what, (*counts, *rows1[len(counts) - 1:]), a, b, kw, code, text)


def h(o):
    return o._h


AWGN_NULL = (OUT0, OUT0, None)  # `in` may be null: the noise alone
AWGN_EXTRA = [("first_index negative, out null", (1,), None, None, dict(first=-1), EINVAL, "first_index is negative"),
              ("first_index negative, count 0", (0,), None, None, dict(first=-1), EINVAL, "first_index is negative"),
              ("first_index negative, count above", (3,), None, None, dict(first=-1), ESIZE, "n_samples exceeds max_samples"),
              ("first_index + count past 2^63 - 1, out null", (2,), None, None, dict(first=(1 << 63) - 2), EINVAL, "first_index + n_samples passes 2^63 - 1")]
ENTRIES = [
    Entry("agc", "work_device", lambda o, c, a, b, said: lib.dvbs2_agc_work_device(h(o), a, S, c[0], c[1], b, S, None, 0, None), "n_samples", "max_samples"),
    Entry("agc", "work", lambda o, c, a, b, said: lib.dvbs2_agc_work(h(o), a, c[0], b, None), "n_samples", "max_samples", rows=False, align=None),
    Entry("awgn", "add_device", lambda o, c, a, b, said, first=0: lib.dvbs2_awgn_add_device(h(o), a, S, c[0], c[1], 0, first, None, b, S, None),
          "n_samples", "max_samples", null=AWGN_NULL, extra=AWGN_EXTRA),
    Entry("awgn", "add", lambda o, c, a, b, said, first=0: lib.dvbs2_awgn_add(h(o), a, c[0], 0, first, b), "n_samples", "max_samples", rows=False,
          null=AWGN_NULL, align=None, extra=AWGN_EXTRA),
    Entry("iqconv", "unpack_device", lambda o, c, a, b, said: lib.dvbs2_iqconv_unpack_device(h(o), a, S, c[0], c[1], b, S, None, None),
          "n_samples", "max_samples", align="out must be 8-byte aligned"),
    Entry("iqconv", "pack_device", lambda o, c, a, b, said: lib.dvbs2_iqconv_pack_device(h(o), a, S, c[0], c[1], b, S, None, None),
          "n_samples", "max_samples", null=(OUT0, OUT0, IN0), align="in must be 8-byte aligned"),
    Entry("iqconv", "unpack_to_device", lambda o, c, a, b, said: lib.dvbs2_iqconv_unpack_to_device(h(o), a, c[0], b, None),
          "n_samples", "max_samples", rows=False, align="out must be 8-byte aligned"),
    Entry("iqconv", "pack_from_device", lambda o, c, a, b, said: lib.dvbs2_iqconv_pack_from_device(h(o), a, c[0], b, None),
          "n_samples", "max_samples", rows=False, null=(OUT0, OUT0, IN0), align="in must be 8-byte aligned"),
    Entry("pulse", "shape_device", lambda o, c, a, b, said: lib.dvbs2_pulse_shape_device(h(o), a, S, c[0], c[1], b, S, None), "n_syms", "max_symbols"),
    Entry("pulse", "shape", lambda o, c, a, b, said: lib.dvbs2_pulse_shape(h(o), a, c[0], b), "n_syms", "max_symbols", rows=False, align=None),
    Entry("resamp", "process_device", lambda o, c, a, b, said: lib.dvbs2_resamp_process_device(h(o), a, S, c[0], c[1], b, S, C.addressof(said), None),
          "n_in", "max_samples"),
    Entry("resamp", "process", lambda o, c, a, b, said, cap=S: lib.dvbs2_resamp_process(h(o), a, c[0], b, cap, C.cast(said, C.POINTER(C.c_int64))),
          "n_in", "max_samples", rows=False, align=None, refused_says=0,
          extra=[("out_cap and count negative", (-1,), R, R, dict(cap=-1), EINVAL, "out_cap is negative")]),
    Entry("ddc", "process_device", lambda o, c, a, b, said: lib.dvbs2_ddc_process_device(h(o), a, S, c[0], c[1], c[2], b, S,
                                                                                         C.cast(said, C.POINTER(C.c_int64)), None), "n_in", "max_samples"),
    Entry("ddc", "process", lambda o, c, a, b, said: lib.dvbs2_ddc_process(h(o), a, S, c[0], c[1], c[2], b, S, C.cast(said, C.POINTER(C.c_int64))),
          "n_in", "max_samples", align=None),
    Entry("spectrum", "process_device", lambda o, c, a, b, said: lib.dvbs2_spectrum_process_device(h(o), a, S, c[0], c[1], b, S,
                                                                                                   C.cast(said, C.POINTER(C.c_int)), None),
          "n_in", "max_samples", top=64, one=64, align="in must be 8-byte aligned",
          extra=[("one sample is no row, null buffers", (1,), None, None, {}, OK, None)]),
    Entry("spectrum", "process", lambda o, c, a, b, said: lib.dvbs2_spectrum_process(h(o), a, S, c[0], c[1], b, S, C.cast(said, C.POINTER(C.c_int))),
          "n_in", "max_samples", top=64, one=64, align=None, extra=[("one sample is no row, null buffers", (1,), None, None, {}, OK, None)]),
]


def test_every_stage_has_its_entries():
    assert {e.stage for e in ENTRIES} == set(STAGES)
    assert R % 8 == 0


@pytest.mark.parametrize("e", ENTRIES, ids=[f"{e.stage}-{e.name}" for e in ENTRIES])
def test_order_of_the_call_checks(e):
    make, good, _ = STAGES[e.stage]
    want = reference(e.stage)
    o = make()
    answers, expected = [], []
    for what, counts, a, b, kw, code, text in e.table():
        said = (C.c_int64 * 2)(SENT, SENT)
        rc = e.call(o, counts, a, b, said, **kw)
        got_text = lib.dvbs2_last_error().decode() if rc else None
        print(f"{e.stage}-{e.name}: {what} {counts}: code {rc} text {got_text!r} says {list(said)}")
        answers.append((what, rc, got_text))
        expected.append((what, code, text))
        if e.stage == "resamp" and e.rows:
            says = [0, SENT] if rc == OK else [SENT, SENT]  # one count per row
        elif e.stage in ("resamp", "ddc", "spectrum"):
            first = 0 if rc == OK else e.refused_says
            says = [first, SENT] if e.stage != "spectrum" else None
            if says is None:  # an int: the low half of the first word
                assert C.cast(said, C.POINTER(C.c_int))[0] == first and C.cast(said, C.POINTER(C.c_int))[1] == -1 and said[1] == SENT, what
        else:
            says = [SENT, SENT]
        if says is not None:
            assert list(said) == says, (what, list(said), says)
        assert (ROOM == FILL).all(), f"{what}: the call wrote to a buffer"
    assert answers == expected
    assert good(o) == want, "behind the refused calls the handle answers differently from a fresh one"
    o.close()


def test_resamp_produce_counts():
    """dvbs2_resamp_produce has the four count checks of the work entries in their order, then its own: somewhere to put the counts"""
    want = reference("resamp")
    o = resamp_make()
    table = [("count negative, rows above", -1, 3, True, EINVAL, "n_in is negative"), ("count above, rows negative", 3, -1, True, EINVAL, "n_streams is negative"),
             ("both above", 3, 3, True, ESIZE, "n_in exceeds max_samples"), ("rows above, nowhere to put the counts", 1, 3, False, ESIZE, "n_streams exceeds max_streams"),
             ("nowhere to put the counts", 0, 1, False, EINVAL, "n_out is null"), ("no rows, nowhere to put the counts", 1, 0, False, OK, None),
             ("count 0", 0, 2, True, OK, None)]
    for what, n_in, n_streams, room, code, text in table:
        said = (C.c_int64 * 2)(SENT, SENT)
        rc = lib.dvbs2_resamp_produce(h(o), n_in, n_streams, C.addressof(said) if room else None)
        got_text = lib.dvbs2_last_error().decode() if rc else None
        print(f"resamp-produce: {what}: code {rc} text {got_text!r} says {list(said)}")
        assert (rc, got_text) == (code, text), what
        assert list(said) == ([0, 0] if what == "count 0" else [SENT, SENT]), what
    assert resamp_good(o) == want
    o.close()
