"""The stream contract of dvbs2_bbdeheader_rows_device on a BUSY non-blocking stream: what tests/test_stream_order_gpu.py applies to every
stage (its docstring and notes/stream_order.md say how), by that file's machinery, for an entry that has no handle.
One row: the records zeroed by a hipMemsetAsync, then two calls over three streams cut in two, each behind asynchronous copies ON THE SAME
STREAM that bring its frames and its offsets -- the destination buffers hold nothing before, so a launch that ran in front of the hold's
end, or in front of its copies, would see no frame at all. Enqueued back to back behind the hold with no host synchronisation, the stream
is still pending behind the last enqueue (the entry did not wait) and every output equals the serialized pass on the null stream, which
is tied to the model (tests/bbdeheader_rows_model.py). Then every refusal of the entry over live buffers: nothing is written."""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest

import bbdeheader_rows_model as BM
import fec_testlib as T
import test_bbdeheader_rows_host as H
import test_stream_order_gpu as SO
from dvbs2rx_amd import BBDEHEADER_STATE, bbdeheader_rows_device, bbdeheader_rows_geometry, capi

pytestmark = pytest.mark.gpu

KBCH, S, MAX_FRAMES = 3072, 3, 64
CUT = (17, 0, 9)  # frames of each stream in the first call; the second brings the rest
D2D = 3           # hipMemcpyDeviceToDevice


@functools.lru_cache(None)
def streams():
    fr = [BM.healthy(KBCH, 30, 61)[1], BM.fuzzed(KBCH, 24, 62)[:20], BM.healthy(KBCH, 9, 63)[1]]
    assert [len(f) for f in fr] == [30, 20, 9]
    return fr


def pieces():
    fr = streams()
    return [[f[:k] for f, k in zip(fr, CUT)], [f[k:] for f, k in zip(fr, CUT)]]


@functools.lru_cache(None)
def runtime():
    rt = T.hip_runtime()
    rt.hipMemsetAsync.restype = C.c_int
    rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return rt


def prep(o):
    g = bbdeheader_rows_geometry(KBCH, S, MAX_FRAMES)
    c = NS(g=g, src=[], state=SO.dev(np.full(S * 256, 0x3C, np.uint8)), work=SO.zeros(g["work_bytes"], "uint8"),
           bb=SO.zeros(MAX_FRAMES * KBCH // 8, "uint8"), off=SO.zeros(S + 1, "int32"),
           out=[SO.dev(np.full(g["out_bytes"], 0xA5, np.uint8)) for _ in range(2)], pko=[SO.dev(np.full(S + 1, -7, np.int32)) for _ in range(2)])
    for piece in pieces():
        bb, off = BM.pack(piece, KBCH // 8)
        c.src.append((SO.dev(bb.reshape(-1)), SO.dev(off)))
    return c


def zero_records(o, c, s):
    assert runtime().hipMemsetAsync(c.state.data_ptr(), 0, S * 256, s or None) == 0


def call(k):
    def f(o, c, s):
        rt = runtime()
        bb, off = c.src[k]
        assert rt.hipMemcpyAsync(c.bb.data_ptr(), bb.data_ptr(), bb.numel(), D2D, s or None) == 0
        assert rt.hipMemcpyAsync(c.off.data_ptr(), off.data_ptr(), 4 * (S + 1), D2D, s or None) == 0
        bbdeheader_rows_device(c.bb.data_ptr(), KBCH, c.off.data_ptr(), S, MAX_FRAMES, c.state.data_ptr(), c.work.data_ptr(), c.g["work_bytes"],
                               c.out[k].data_ptr(), c.g["out_bytes"], c.pko[k].data_ptr(), 0, s)
    return f


def collect(o, c):
    return dict(state=SO.host(c.state), out0=SO.host(c.out[0]), out1=SO.host(c.out[1]), pko0=SO.host(c.pko[0]), pko1=SO.host(c.pko[1]))


def model(got):
    m = BM.Rows(KBCH, S)
    for k, piece in enumerate(pieces()):
        want, want_pko = m.call(piece)
        assert got[f"pko{k}"].tolist() == want_pko, k
        ts = np.concatenate(want)
        assert np.array_equal(got[f"out{k}"][:ts.size], ts) and (got[f"out{k}"][ts.size:] == 0xA5).all(), f"call {k}: the serialized pass is not the model"
    assert BM.canon(got["state"].view(BBDEHEADER_STATE)).tobytes() == BM.canon(m.records()).tobytes()
    assert m.counters()[0]["packets"] > 50 and m.counters()[1]["bbframes"] == 20  # stream 1 was not touched by the first call and was by the second


@functools.lru_cache(None)
def the_row():
    return SO.Row("bbdeheader_rows", (), lambda: (), prep, [zero_records, call(0), call(1)], collect, model)


@functools.lru_cache(None)
def reference():
    """as test_stream_order_gpu.reference: the serialized pass twice, the first checked against the model"""
    row = the_row()
    want, _ = SO.run_serialized(row)
    row.model(want)
    again, spent = SO.run_serialized(row)
    SO.same(again, want, "bbdeheader_rows: the serialized pass, repeated")
    return want, spent * 1e3


def test_pending_calls_equal_the_serialized_ones():
    want, host_ms = reference()
    hold_ms = T.hold_for(host_ms)
    print(f"stream-order: bbdeheader_rows: host side of the enqueues {host_ms:.3f} ms, hold {hold_ms:.0f} ms")
    got = SO.run_held(the_row(), T.side_stream(), hold_ms)
    SO.same(got, want, "bbdeheader_rows: behind a hold")


def test_refused_calls_write_nothing():
    """the refusals of tests/test_bbdeheader_rows_host.py with live buffers behind every pointer that is not the one refused, and a device
    that does not exist behind arguments that pass: records, workspace, output and pkt_offsets keep their bytes"""
    import torch
    c = prep(())
    torch.cuda.synchronize()
    before = {k: SO.host(t).tobytes() for k, t in (("state", c.state), ("work", c.work), ("out", c.out[0]), ("pko", c.pko[0]))}
    g = c.g
    live = (c.bb.data_ptr(), KBCH, c.off.data_ptr(), S, MAX_FRAMES, c.state.data_ptr(), c.work.data_ptr(), g["work_bytes"], c.out[0].data_ptr(), g["out_bytes"],
            c.pko[0].data_ptr())
    good = H.good_rows()
    n = 0
    for a, code, text in H.rows_refused():
        changed = {name: v for name, v, w in zip(H.ROWS_NAMES, a, good) if v != w and name not in ("work_bytes", "out_bytes")}
        b = H.with_(live, **changed)
        if a[7] != good[7]:
            b = H.with_(b, work_bytes=a[7] - good[7] + g["work_bytes"])
        if a[9] != good[9]:
            b = H.with_(b, out_bytes=a[9] - good[9] + g["out_bytes"])
        assert H.rows_call(b) == code, (text, capi.lib.dvbs2_last_error())
        # (the sizes of this geometry are not that file's: the text up to the number)
        assert capi.lib.dvbs2_last_error().decode().startswith(text if code == capi.EINVAL else text.rsplit(" ", 1)[0] + " ")
        n += 1
    assert n == len(H.rows_refused()) >= 20
    T.refused(capi.EINVAL, "device index out of range", capi.lib.dvbs2_bbdeheader_rows_device, *live, 1 << 20, None)
    torch.cuda.synchronize()
    after = {k: SO.host(t).tobytes() for k, t in (("state", c.state), ("work", c.work), ("out", c.out[0]), ("pko", c.pko[0]))}
    assert after == before
