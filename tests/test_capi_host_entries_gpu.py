"""Host-buffer entry == device entry, for each of the nine stage handles (bch, demap, plpayload, plframe, plsync, plcoarse, rotator,
symsync, bbdeheader).

A host-buffer entry stages the caller's buffers in device memory the handle keeps, runs the *_device entry on a stream of its own and
copies the results back. Each test here runs the same sequence of calls through both forms, each on a handle of its own (several stages
keep state between calls), and compares every output byte for byte: the two forms run the same kernels on the same input, so there is no
reference and no tolerance. The sequences reuse the staging (3 frames, then 4 with max_frames = 4), include the call that does nothing
(0 frames) and the one that is refused (max_frames + 1: DVBS2_ESIZE), and, for the two handles whose staging grows on demand, go
64 -> 4096 -> 64 samples."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import BbDeheader, BchDecoder, Demapper, PlCoarse, PlFrontEnd, PlPayload, PlSync, Rotator, SymbolSync, capi
from dvbs2rx_amd.capi import lib

pytestmark = pytest.mark.gpu

MF = 4
SHORT = capi.FECFRAME_SHORT
SEQUENCE = (3, 4, 0, MF + 1, 4)  # frames per call, on one handle


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def ptr(x):
    return None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def same(host, device, what):
    import torch
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(host, device)):
        if a is not None:
            assert a.tobytes() == b.cpu().numpy().tobytes(), f"{what}: output {i} of the host entry differs from the device entry's"


def run_frames(make, inputs, outputs, host, device):
    """make() -> handle object; inputs(n, call) / outputs(n) -> lists of numpy arrays (None: absent); host(obj, n, ins, outs) and
    device(obj, n, d_ins, d_outs, stream) -> DVBS2 code. Runs SEQUENCE on a handle per form."""
    hobj, dobj = make(), make()
    for call, n in enumerate(SEQUENCE):
        ins, outs = inputs(n, call), outputs(n)
        d_ins = [None if a is None else dev(a) for a in ins]
        d_outs = [None if a is None else dev(a) for a in outputs(n)]
        before = [None if a is None else a.copy() for a in outs]
        rc_h, rc_d = host(hobj, n, ins, outs), device(dobj, n, d_ins, d_outs, T.stream())
        want = capi.ESIZE if n > MF else capi.OK
        assert (rc_h, rc_d) == (want, want), (call, n, rc_h, rc_d, lib.dvbs2_last_error())
        if n > MF:
            assert b"max_frames" in lib.dvbs2_last_error()
        if n == 0 or n > MF:
            assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(outs, before)), f"call {call} ({n} frames) wrote to an output"
        else:
            same(outs, d_outs, f"call {call} ({n} frames)")
    hobj.close()
    dobj.close()
    make().close()  # the device is as it was: a following create works


def filled(shape, dtype):
    return np.full(shape, 90, dtype)  # what an output holds before the call


def rng_of(*key):
    return np.random.default_rng(list(key))


# ------------------------------------------------------------------ bch
def test_bch():
    make = lambda: BchDecoder(framesize=SHORT, rate="C1_4", max_frames=MF)
    probe = make()
    nb, kb = probe.n // 8, probe.k // 8
    probe.close()

    def inputs(n, call):  # the all-zero codeword with up to three bit errors per frame
        rng, cw = rng_of(1, call), np.zeros((max(n, 1), nb), np.uint8)
        for f in range(n):
            for pos in rng.integers(0, nb * 8, f % 4):
                cw[f, pos // 8] ^= 0x80 >> (pos % 8)
        return [cw]

    outputs = lambda n: [filled((max(n, 1), kb), np.uint8), filled(max(n, 1), np.int32)]
    run_frames(make, inputs, outputs,
               lambda o, n, i, r: lib.dvbs2_bch_decode(o._h, ptr(i[0]), n, ptr(r[0]), ptr(r[1])),
               lambda o, n, i, r, st: lib.dvbs2_bch_decode_device(o._h, ptr(i[0]), n, ptr(r[0]), ptr(r[1]), st))


# ------------------------------------------------------------------ demapper: QPSK, and 16APSK on the 4050-symbol short frame
@pytest.mark.parametrize("rate,constellation", [("C1_4", capi.MOD_QPSK), ("C2_3", capi.MOD_16APSK)])
def test_demap(rate, constellation):
    make = lambda: Demapper(framesize=SHORT, rate=rate, constellation=constellation, max_frames=MF)
    probe = make()
    ns, nl = probe.n_syms, probe.n_llr
    probe.close()
    assert constellation == capi.MOD_QPSK or ns == 4050

    def inputs(n, call):
        rng, m = rng_of(2, call), max(n, 1)
        syms = (rng.normal(size=(m, ns)) + 1j * rng.normal(size=(m, ns))).astype(np.complex64)
        return [syms, rng.uniform(0.05, 0.5, m).astype(np.float32), rng.integers(-127, 128, (m, nl)).astype(np.int8)]

    run_frames(make, inputs, lambda n: [filled((max(n, 1), nl), np.int8)],
               lambda o, n, i, r: lib.dvbs2_demap_soft(o._h, ptr(i[0]), n, ptr(i[1]), n, ptr(r[0])),
               lambda o, n, i, r, st: lib.dvbs2_demap_soft_device(o._h, ptr(i[0]), n, ptr(i[1]), n, ptr(r[0]), st))
    run_frames(make, inputs, lambda n: [filled(max(n, 1), np.float32)],
               lambda o, n, i, r: lib.dvbs2_demap_estimate_snr(o._h, ptr(i[0]), n, ptr(r[0])),
               lambda o, n, i, r, st: lib.dvbs2_demap_estimate_snr_device(o._h, ptr(i[0]), n, ptr(r[0]), st))
    run_frames(make, inputs, lambda n: [filled(max(n, 1), np.float32)],
               lambda o, n, i, r: lib.dvbs2_demap_refine_snr(o._h, ptr(i[0]), ptr(i[2]), n, ptr(r[0])),
               lambda o, n, i, r, st: lib.dvbs2_demap_refine_snr_device(o._h, ptr(i[0]), ptr(i[2]), n, ptr(r[0]), st))


# ------------------------------------------------------------------ PLFRAME payload step
def test_plpayload():
    make = lambda: PlPayload(gold_code=0, n_slots=90, has_pilots=True, max_frames=MF)
    probe = make()
    pl, xl, npil = probe.payload_len, probe.xfecframe_len, probe.n_pilots
    probe.close()
    assert npil > 0

    def inputs(n, call):
        rng, m = rng_of(3, call), max(n, 1)
        return [(rng.normal(size=(m, pl)) + 1j * rng.normal(size=(m, pl))).astype(np.complex64), rng.uniform(-3, 3, m).astype(np.float32),
                rng.uniform(-1e-3, 1e-3, m).astype(np.float32), rng.integers(0, 2, m).astype(np.int32),
                rng.uniform(-3, 3, (m, npil)).astype(np.float32)]

    run_frames(make, inputs, lambda n: [filled((max(n, 1), xl), np.complex64)],
               lambda o, n, i, r: lib.dvbs2_plpayload_process(o._h, ptr(i[0]), n, ptr(i[1]), ptr(i[2]), ptr(i[3]), ptr(i[4]), ptr(r[0])),
               lambda o, n, i, r, st: lib.dvbs2_plpayload_process_device(o._h, ptr(i[0]), n, ptr(i[1]), ptr(i[2]), ptr(i[3]), ptr(i[4]), ptr(r[0]), st))


# ------------------------------------------------------------------ PLFRAME front end: with pilots (no coarse_foffset) and without (needs it)
@pytest.mark.parametrize("pilots", [1, 0])
@pytest.mark.parametrize("process", [False, True])
def test_plframe(pilots, process):
    plsc = P.plsc_of(4, 1, pilots)
    make = lambda: PlFrontEnd(gold_code=0, plsc=plsc, max_frames=MF)
    probe = make()
    fl, xl, npil = probe.plframe_len, probe.xfecframe_len, probe.n_pilots
    probe.close()
    assert (npil > 0) == bool(pilots)

    def inputs(n, call):
        rng, m = rng_of(4, call, pilots), max(n, 1)
        frames, _ = M.make_plframes(plsc, 0, m, rng, es_n0_db=8.0, phase=0.3, foffset=1e-4)
        cf = None if pilots else rng.uniform(-1e-3, 1e-3, m).astype(np.float32)
        return [np.ascontiguousarray(frames.reshape(m, fl), np.complex64), np.ones(m, np.int32), cf]

    def outputs(n):
        m = max(n, 1)
        est = [filled(m, np.uint8), filled(m, np.float32), filled(m, np.float32), filled((m, npil), np.float32) if npil else None,
               filled(m, np.float32), filled(m, np.int32)]  # the order of capi.PlFrameEstimates
        return [filled((m, xl), np.complex64) if process else None] + est

    def est_of(r):
        return C.byref(capi.PlFrameEstimates(*[ptr(a) for a in r[1:]]))

    if process:
        host = lambda o, n, i, r: lib.dvbs2_plframe_process(o._h, ptr(i[0]), n, 0, ptr(i[1]), ptr(i[2]), ptr(r[0]), est_of(r))
        device = lambda o, n, i, r, st: lib.dvbs2_plframe_process_device(o._h, ptr(i[0]), n, 0, ptr(i[1]), ptr(i[2]), ptr(r[0]), est_of(r), st)
    else:
        host = lambda o, n, i, r: lib.dvbs2_plframe_estimate(o._h, ptr(i[0]), n, 0, ptr(i[1]), ptr(i[2]), est_of(r))
        device = lambda o, n, i, r, st: lib.dvbs2_plframe_estimate_device(o._h, ptr(i[0]), n, 0, ptr(i[1]), ptr(i[2]), est_of(r), st)
    run_frames(make, inputs, outputs, host, device)


# ------------------------------------------------------------------ coarse frequency estimate (keeps its window between calls)
def test_plcoarse():
    make = lambda: PlCoarse(period=2, plsc=-1, max_frames=MF)

    def inputs(n, call):
        rng, m = rng_of(5, call), max(n, 1)
        plsc = rng.integers(0, 128, m).astype(np.uint8)
        hdr = np.stack([M.plheader(int(p)) for p in plsc]) * np.exp(2j * np.pi * 0.01 * np.arange(90))
        x = np.concatenate([hdr, P.qpsk(rng, m * 10).reshape(m, 10)], axis=1)  # stride 100: the 2-D staging copy
        return [np.ascontiguousarray(x, np.complex64), plsc]

    outputs = lambda n: [filled(max(n, 1), np.float32), filled(max(n, 1), np.int32), filled(max(n, 1), np.int32)]
    run_frames(make, inputs, outputs,
               lambda o, n, i, r: lib.dvbs2_plcoarse_estimate(o._h, ptr(i[0]), 100, ptr(i[1]), n, ptr(r[0]), ptr(r[1]), ptr(r[2])),
               lambda o, n, i, r, st: lib.dvbs2_plcoarse_estimate_device(o._h, ptr(i[0]), 100, ptr(i[1]), n, ptr(r[0]), ptr(r[1]), ptr(r[2]), st))


# ------------------------------------------------------------------ BBFRAME de-header (keeps the partial packet between calls)
def test_bbdeheader():
    import torch
    make = lambda: BbDeheader(framesize=SHORT, rate="C1_4", max_frames=MF)
    hobj, dobj = make(), make()
    kbch, ob = hobj.kbch_bytes * 8, hobj.max_out_bytes_per_frame
    total = sum(n for n in SEQUENCE if n <= MF)
    frames = T.bbframe_stream(kbch, total, T.ts_up_stream(-(-total * (kbch - 80) // (8 * 188)), rng_of(6)), 0)
    at, produced_total = 0, 0
    for call, n in enumerate(SEQUENCE):
        x = np.ascontiguousarray(frames[at:at + n]) if n <= MF else np.zeros((n, kbch // 8), np.uint8)
        out, d_x, d_out = filled(max(n, 1) * ob, np.uint8), dev(x if n else np.zeros(8, np.uint8)), dev(filled(max(n, 1) * ob, np.uint8))
        got = C.c_int64(-1)
        rc_h = lib.dvbs2_bbdeheader_process(hobj._h, ptr(x), n, ptr(out), C.byref(got))
        rc_d = lib.dvbs2_bbdeheader_process_device(dobj._h, ptr(d_x), n, ptr(d_out), T.stream())
        want = capi.ESIZE if n > MF else capi.OK
        assert (rc_h, rc_d) == (want, want), (call, n, rc_h, rc_d, lib.dvbs2_last_error())
        if n > MF:
            assert got.value == -1 and not (out != 90).any()
            continue
        at += n
        k = dobj.finish(T.stream())
        torch.cuda.synchronize()
        assert got.value == k and out[:k].tobytes() == d_out.cpu().numpy()[:k].tobytes(), (call, n, got.value, k)
        assert not (out[k:] != 90).any()
        assert (n > 0) or k == 0
        produced_total += k
    assert produced_total > 0 and hobj.counters() == dobj.counters()
    hobj.close()
    dobj.close()
    make().close()


# ------------------------------------------------------------------ PLFRAME search: two frames in one stream
def test_plsync():
    import torch
    x, sofs, _ = P.make_stream([P.SHORT_QPSK, P.SHORT_QPSK], 7, offset=500)
    make = lambda: PlSync(plsc=-1, max_symbols=max(x.size, PlSync.MIN_SYMBOLS), max_frames=16)
    hobj, dobj = make(), make()
    for call, part in enumerate((x, x[:0], x)):  # the second presentation of the stream finds the handle locked
        recs, consumed, state = hobj.work(part)
        d_x, d_f = dev(part) if part.size else torch.zeros(2, device="cuda"), torch.zeros(16 * 16, dtype=torch.uint8, device="cuda")
        dobj.work_device(d_x.data_ptr(), part.size, d_f.data_ptr(), T.stream())
        nf, d_consumed, d_state = dobj.finish()
        assert (len(recs), consumed, state) == (nf, d_consumed, d_state), call
        assert recs.tobytes() == d_f.cpu().numpy().view(PlSync.FRAME_DTYPE)[:nf].tobytes(), call
        assert nf > 0 if call == 0 else nf == 0 or call == 2, (call, nf)
    assert lib.dvbs2_plsync_search(hobj._h, ptr(x), hobj.max_symbols + 1, ptr(np.zeros(16, PlSync.FRAME_DTYPE)), None, None, None) == capi.ESIZE
    assert b"max_symbols" in lib.dvbs2_last_error()
    hobj.close()
    dobj.close()
    make().close()


# ------------------------------------------------------------------ the handles whose staging grows on demand
GROW = (64, 4096, 64)


def test_rotator():
    import torch
    hobj, dobj = Rotator(phase_inc=0.01), Rotator(phase_inc=0.01)
    for call, n in enumerate(GROW):
        x = P.qpsk(rng_of(8, call), n).astype(np.complex64)
        out = hobj.work(x)
        d_x, d_out = dev(x), torch.zeros(2 * n, device="cuda")
        dobj.work_device(d_x.data_ptr(), n, d_out.data_ptr(), T.stream())
        torch.cuda.synchronize()
        assert out.tobytes() == d_out.cpu().numpy().tobytes(), (call, n)
    assert hobj.position() == dobj.position() == (sum(GROW), 0)
    assert hobj.work(np.zeros(0, np.complex64)).size == 0
    hobj.close()
    dobj.close()
    Rotator().close()


def test_symsync():
    import torch
    make = lambda: SymbolSync(sps=2, max_streams=1, max_samples=8192)
    hobj, dobj = make(), make()
    for call, n in enumerate(GROW):
        rng = rng_of(9, call)
        x = (np.repeat(P.qpsk(rng, n // 2), 2) + 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)
        syms, idx, mu, consumed, status = hobj.work(x)
        d_x, d_out = dev(x), torch.zeros(2 * n, device="cuda")
        d_idx, d_mu = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
        dobj.work_device(d_x.data_ptr(), n, [n], d_out.data_ptr(), n, n, d_idx.data_ptr(), d_mu.data_ptr(), T.stream())
        k, d_consumed, d_status = (int(v[0]) for v in dobj.finish())
        assert (len(syms), consumed, status) == (k, d_consumed, d_status), (call, n)
        assert syms.tobytes() == d_out.cpu().numpy()[:2 * k].tobytes(), (call, n)
        assert idx.tobytes() == d_idx.cpu().numpy()[:k].tobytes() and mu.tobytes() == d_mu.cpu().numpy()[:k].tobytes(), (call, n)
    assert hobj.state() == dobj.state()
    assert lib.dvbs2_symsync_work(hobj._h, ptr(np.zeros(2, np.float32)), 8193, None, 0, None, None, None, None, None) == capi.ESIZE
    assert b"max_samples" in lib.dvbs2_last_error()
    hobj.close()
    dobj.close()
    make().close()


# ------------------------------------------------------------------ a handle that never saw a host entry
def test_create_destroy_without_a_host_entry():
    for _ in range(2):
        for make in (lambda: BchDecoder(framesize=SHORT, rate="C1_4", max_frames=MF), lambda: Demapper(framesize=SHORT, rate="C1_4", max_frames=MF),
                     lambda: PlPayload(n_slots=90, max_frames=MF), lambda: PlFrontEnd(plsc=P.SHORT_QPSK, max_frames=MF),
                     lambda: PlSync(max_symbols=PlSync.MIN_SYMBOLS, max_frames=16), lambda: PlCoarse(max_frames=MF), lambda: Rotator(),
                     lambda: SymbolSync(max_samples=8192), lambda: BbDeheader(framesize=SHORT, rate="C1_4", max_frames=MF)):
            make().close()
