"""Spectrum estimate on the device (dvbs2_spectrum_*). Every output row is compared BIT FOR BIT (uint32; a NaN equals a NaN) with the
float32 restatement of tests/spectrum_model.py over the library's twiddle table, into sentinel-filled buffers whose pads and gaps must
stay untouched, with zeros of both signs and denormals planted in the input, for every nfft (each is a pass plan of its own), hops
below, at and above nfft, rows inside and across the chunk of 16 segments and both bin orders; the device against float64 under the
derived bound; refusals; and a closed loop: two carriers nobody told the receiver about, found in the spectrum and received through
the down-converter with settings derived from the finder's records alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import pulse_model as PM
import spectrum_model as SM
from dvbs2rx_amd import (Agc, Awgn, Ddc, PlCoarse, PulseShaper, Rotator, Spectrum, SymbolSync, awgn_sigma, capi, plframer_layout, pulse_taps,
                         spectrum_carriers, spectrum_geometry, spectrum_twiddles, spectrum_window)
from fec_testlib import PAD, SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu

NFFTS = [1 << t for t in range(6, 14)]


@functools.lru_cache(maxsize=None)
def table(nfft):
    return spectrum_twiddles(nfft)


@functools.lru_cache(maxsize=None)
def hann(nfft):
    return spectrum_window("hann", nfft)


@functools.lru_cache(maxsize=None)
def data(seed, n):
    x = PM.planted(np.random.default_rng(seed), n)
    x.setflags(write=False)
    return x


def run_on_device(sp, xs, in_stride=None, out_stride=None, in_shift=0, out_shift=0):
    """One work_device call over the streams xs (complex64 vectors of one length n). Stream i lies at in_shift + i * in_stride complex
    elements of a 16-byte-aligned buffer and writes at out_shift + i * out_stride FLOATS of a 16-byte-aligned sentinel buffer. Returns
    one uint32 [n_rows, nfft] array per stream after checking the reported row count against the geometry, that everything else in
    the output buffer is still the sentinel, and that the input is unchanged."""
    import torch
    ns, n = len(xs), xs[0].size
    n_rows = sp.geometry(n)[1]
    count = n_rows * sp.nfft
    in_stride = max(n, 1) if in_stride is None else in_stride
    out_stride = max(count, 1) if out_stride is None else out_stride
    host_in = np.full(in_shift + ns * in_stride + 2, np.complex64(complex(9.5, -9.5)), np.complex64)
    for i, x in enumerate(xs):
        assert x.size == n
        host_in[in_shift + i * in_stride:in_shift + i * in_stride + n] = x
    d_in = torch.from_numpy(host_in.view(np.float32)).cuda()
    n_buf = out_shift + ns * out_stride + PAD
    d_out = sentinel(n_buf)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    said = sp.work_device(d_in.data_ptr() + 8 * in_shift, in_stride, n, ns, d_out.data_ptr() + 4 * out_shift, out_stride, stream())
    torch.cuda.synchronize()
    assert said == n_rows == SM.geometry(sp.nfft, sp.hop, sp.avg, n)[1]
    got = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), host_in.view(np.uint32)), "the input was written"
    touched = np.zeros(n_buf, bool)
    outs = []
    for i in range(ns):
        a = out_shift + i * out_stride
        touched[a:a + count] = True
        outs.append(got[a:a + count].reshape(n_rows, sp.nfft))
    assert (got[~touched] == SENTINEL).all(), "a write outside the rows"
    return outs


def same(got, want, what):
    """got: uint32 rows from the device; want: the model's float32 rows. The same bits; where the model has a NaN the device has one
    (the payload of a NaN that an operation creates is the processor's own: x86 sets the sign bit, the GPU does not)."""
    w = np.ascontiguousarray(want, np.float32)
    assert got.shape == w.shape, (what, got.shape, w.shape)
    g = got.view(np.float32)
    ok = (got == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    if not ok.all():
        bad = np.argwhere(~ok)
        r, k = bad[0]
        raise AssertionError(f"{what}: {bad.shape[0]} of {w.size} bins differ, the first at row {r} bin {k}: {g[r, k]!r} != {w[r, k]!r}")


def n_in_for(nfft, hop, n_seg):
    """the longest input with exactly n_seg segments: the last hop - 1 samples belong to no segment"""
    return nfft + (n_seg - 1) * hop + hop - 1


# ------------------------------------------------------------------ 1. bit for bit
SEGS_OF_AVG = {0: 33, 1: 3, 2: 5, 16: 33, 17: 35}  # one row of 3 chunks; rows of 1; 2 rows and a segment over; 2 rows of a chunk; 2 rows of 16 + 1


@pytest.mark.parametrize("nfft", NFFTS)
def test_bit_for_bit(nfft):
    """Hops of nfft, nfft / 2, 37 and nfft + 5, avg in {0, 1, 2, 16, 17} (16 and 17 straddle the chunk, avg = 0 runs 33 segments), both
    bin orders: every row equals the model's, and the shifted row is fftshift of the unshifted one."""
    w = hann(nfft)
    for hop in (nfft, nfft // 2, 37, nfft + 5):
        for avg, n_seg in SEGS_OF_AVG.items():
            n = n_in_for(nfft, hop, n_seg)
            assert spectrum_geometry(nfft, hop, avg, n)[0] == n_seg
            x = data(nfft + hop + avg, n)
            want = SM.rows32(x, nfft, hop, avg, w, table(nfft), False)
            assert want.shape[0] == (1 if avg == 0 else n_seg // avg)
            rows = {}
            for shifted in (False, True):
                sp = Spectrum(nfft, hop, avg, w, shifted, max_samples=n)
                assert (sp.nfft, sp.hop, sp.avg, sp.shifted, sp.window_power) == (nfft, hop, avg, shifted, SM.window_power(w))
                rows[shifted] = run_on_device(sp, [x])[0]
                sp.close()
            same(rows[False], want, f"nfft {nfft} hop {hop} avg {avg}")
            assert np.array_equal(np.fft.fftshift(rows[False], axes=-1), rows[True]), (nfft, hop, avg)


@pytest.mark.parametrize("nfft", NFFTS)
def test_overflow_nonfinite_and_denormals(nfft):
    """Values near 1e19 on part of the input so that some powers overflow to infinity and others do not, an infinite and a NaN sample
    (NaNs through inf - inf and 0 inf in the butterflies), and an input so small that powers, sums and scaled rows are denormal:
    infinities, NaNs and denormals are where the model has them. A null window is the Hann window."""
    hop, n_seg = nfft // 2, 20
    n = n_in_for(nfft, hop, n_seg)
    big = np.array(data(77, n))
    big[nfft:3 * nfft] *= np.float32(1e19)
    big[7 * hop + 5] = np.complex64(complex(np.inf, 1.0))
    big[12 * hop + 9] = np.complex64(complex(2.0, np.nan))
    tiny = np.array(data(78, n)) * np.float32(1e-21)
    for avg in (2, 0):
        sp = Spectrum(nfft, hop, avg, None, False, max_samples=n)
        for x, what in ((big, "big"), (tiny, "tiny")):
            want = SM.rows32(x, nfft, hop, avg, hann(nfft), table(nfft), False)
            got = run_on_device(sp, [x])[0]
            same(got, want, f"nfft {nfft} avg {avg} {what}")
            if what == "big" and avg == 2:
                assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
            if what == "tiny":
                assert ((want > 0) & (want < np.finfo(np.float32).tiny)).any()
        sp.close()


def test_other_windows_and_rect():
    nfft, hop, avg = 256, 100, 3
    n = n_in_for(nfft, hop, 7)
    x = data(5, n)
    for kind in ("rect", "hamming", "blackman-harris"):
        w = spectrum_window(kind, nfft)
        sp = Spectrum(nfft, hop, avg, kind, True, max_samples=n)
        same(run_on_device(sp, [x])[0], SM.rows32(x, nfft, hop, avg, w, table(nfft), True), kind)
        sp.close()


# ------------------------------------------------------------------ 2. batches and layout
def test_streams_and_strides():
    """3 streams with in_stride > n_in and out_stride > n_rows nfft, rows of one and of several chunks."""
    nfft, hop = 512, 256
    for avg, n_seg in ((0, 20), (4, 9)):
        n = n_in_for(nfft, hop, n_seg)
        xs = [data(100 + i, n) for i in range(3)]
        sp = Spectrum(nfft, hop, avg, None, True, max_streams=3, max_samples=n)
        got = run_on_device(sp, xs, in_stride=n + 3, out_stride=sp.geometry(n)[1] * nfft + 5)
        for i in range(3):
            same(got[i], SM.rows32(xs[i], nfft, hop, avg, hann(nfft), table(nfft), True), f"stream {i} avg {avg}")
        assert not np.array_equal(got[0], got[1])
        sp.close()


def test_300_streams_of_one_segment():
    nfft = 64
    xs = [data(200 + i, nfft) for i in range(300)]
    for avg in (0, 1):
        sp = Spectrum(nfft, nfft, avg, None, False, max_streams=300, max_samples=nfft)
        got = run_on_device(sp, xs)
        for i in (0, 1, 17, 255, 256, 299):
            same(got[i], SM.rows32(xs[i], nfft, nfft, avg, hann(nfft), table(nfft), False), f"stream {i}")
        want = np.stack([SM.rows32(x, nfft, nfft, avg, hann(nfft), table(nfft), False)[0] for x in xs])
        same(np.concatenate(got), want, "300 streams")
        sp.close()


@pytest.mark.parametrize("in_shift", (0, 1))
@pytest.mark.parametrize("out_shift", (0, 1, 2, 3))
def test_alignment(in_shift, out_shift):
    """The input at both 8-byte phases of a 16-byte line, the output at every 4-byte phase: the same bits."""
    for nfft, avg, n_seg in ((128, 0, 19), (2048, 2, 4)):
        hop = nfft // 2
        n = n_in_for(nfft, hop, n_seg)
        xs = [data(300, n), data(301, n)]
        sp = Spectrum(nfft, hop, avg, None, True, max_streams=2, max_samples=n)
        got = run_on_device(sp, xs, in_stride=n + 1, out_stride=sp.geometry(n)[1] * nfft + 1, in_shift=in_shift, out_shift=out_shift)
        for i in range(2):
            same(got[i], SM.rows32(xs[i], nfft, hop, avg, hann(nfft), table(nfft), True), f"nfft {nfft} stream {i}")
        sp.close()


def test_short_inputs_write_nothing():
    import torch
    nfft = 256
    for avg, n in ((0, nfft - 1), (0, 0), (4, nfft + 3 * 128 - 1)):  # no segment; nothing at all; three segments where a row takes four
        sp = Spectrum(nfft, 128, avg, None, True, max_streams=2, max_samples=4096)
        assert sp.geometry(n)[1] == 0
        assert run_on_device(sp, [data(1, max(n, 1))[:n], data(2, max(n, 1))[:n]], in_stride=max(n, 1), out_stride=8)[0].shape == (0, nfft)
        rows = C.c_int(-7)
        assert capi.lib.dvbs2_spectrum_process_device(sp._h, None, 0, n, 2, None, 0, C.byref(rows), stream()) == capi.OK and rows.value == 0
        assert sp.work(np.zeros((2, n), np.complex64)).shape == (2, 0, nfft)
        sp.close()
    torch.cuda.synchronize()


def test_host_entry_equals_the_device_entry():
    for nfft, hop, avg, n_seg in ((64, 32, 0, 40), (1024, 512, 3, 7), (8192, 4096, 0, 3)):
        n = n_in_for(nfft, hop, n_seg)
        xs = np.stack([data(400, n), data(401, n)])
        sp = Spectrum(nfft, hop, avg, None, True, max_streams=2, max_samples=n)
        got = sp.work(xs)
        assert got.dtype == np.float32 and got.shape == (2, sp.geometry(n)[1], nfft)
        dev = run_on_device(sp, [xs[0], xs[1]])
        for i in range(2):
            assert np.array_equal(got[i].view(np.uint32), dev[i]), (nfft, i)
        one = sp.work(xs[1])
        assert np.array_equal(one[0].view(np.uint32), dev[1])
        sp.close()


# ------------------------------------------------------------------ 3. accuracy
@pytest.mark.parametrize("nfft", (64, 1024, 8192))
def test_accuracy_against_the_float64_reference(nfft):
    """|device - float64| per bin is within the bound of spectrum_model.rows64: Higham's Theorem 24.2 for the transform, carried through
    the window product, the power, the two-level sum and the scale (notes/spectrum.md)."""
    rng = np.random.default_rng(nfft + 1)
    hop = nfft // 2
    n = n_in_for(nfft, hop, 17)
    x = (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)
    for avg in (0, 4):
        sp = Spectrum(nfft, hop, avg, None, False, max_samples=n)
        got = run_on_device(sp, [x])[0].view(np.float32).astype(np.float64)
        want, bound = SM.rows64(x, nfft, hop, avg, hann(nfft), table(nfft), False)
        ratio = (np.abs(got - want) / bound).max()
        print(f"nfft {nfft} avg {avg}: worst error / bound {ratio:.4f}, worst relative error {(np.abs(got - want) / want).max():.3e}")
        assert ratio <= 1.0
        sp.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals_leave_everything_untouched():
    import torch
    lib, h = capi.lib, C.c_void_p()
    create = lib.dvbs2_spectrum_create
    w = hann(64).copy()
    for nfft in (0, 32, 96, 16384):
        refused(capi.EINVAL, "nfft must be a power of two in 64..8192", create, C.byref(h), nfft, 32, 0, None, 1, 1, 1000, 0)
    refused(capi.EINVAL, "hop must be in 1..2^24", create, C.byref(h), 64, 0, 0, None, 1, 1, 1000, 0)
    refused(capi.EINVAL, "hop must be in 1..2^24", create, C.byref(h), 64, (1 << 24) + 1, 0, None, 1, 1, 1000, 0)
    refused(capi.EINVAL, "avg is negative", create, C.byref(h), 64, 32, -1, None, 1, 1, 1000, 0)
    bad = w.copy()
    bad[9] = np.inf
    refused(capi.EINVAL, "window[9] is not finite", create, C.byref(h), 64, 32, 0, bad.ctypes.data, 1, 1, 1000, 0)
    bad[9] = np.nan
    refused(capi.EINVAL, "window[9] is not finite", create, C.byref(h), 64, 32, 0, bad.ctypes.data, 1, 1, 1000, 0)
    zeros = np.zeros(64, np.float32)
    refused(capi.EINVAL, "the window is all zero", create, C.byref(h), 64, 32, 0, zeros.ctypes.data, 1, 1, 1000, 0)
    refused(capi.EINVAL, "max_streams out of range (1..65535)", create, C.byref(h), 64, 32, 0, None, 1, 0, 1000, 0)
    refused(capi.EINVAL, "max_samples out of range (1..2^24)", create, C.byref(h), 64, 32, 0, None, 1, 1, (1 << 24) + 1, 0)
    refused(capi.EINVAL, "null handle pointer", create, None, 64, 32, 0, None, 1, 1, 1000, 0)
    assert not h
    assert create(C.byref(h), 64, 32, 0, None, 1, 1, 1000, 99) < 0 and not h  # no such device
    # the null handle, for every entry that takes one
    rows = C.c_int(-7)
    r = C.byref(rows)
    lib.dvbs2_spectrum_destroy(None)
    refused(capi.EINVAL, "null handle", lib.dvbs2_spectrum_params, None, None, None, None, None, None)
    refused(capi.EINVAL, "null handle", lib.dvbs2_spectrum_process_device, None, None, 0, 0, 0, None, 0, r, None)
    refused(capi.EINVAL, "null handle", lib.dvbs2_spectrum_process, None, None, 0, 0, 0, None, 0, r)

    nfft, hop, avg = 64, 32, 2
    n = n_in_for(nfft, hop, 5)
    sp = Spectrum(nfft, hop, avg, None, True, max_streams=2, max_samples=n)
    n_rows = sp.geometry(n)[1]
    assert n_rows == 2
    xs = [data(500, n), data(501, n)]
    d_in = torch.from_numpy(np.concatenate(xs).view(np.float32)).cuda()
    d_out = sentinel(2 * n_rows * nfft + PAD)
    st = stream()
    a, o, stride = d_in.data_ptr(), d_out.data_ptr(), n_rows * nfft
    entry = lib.dvbs2_spectrum_process_device
    refused(capi.ESIZE, "n_in exceeds max_samples", entry, sp._h, a, n + 1, n + 1, 2, o, stride, r, st)
    refused(capi.ESIZE, "n_streams exceeds max_streams", entry, sp._h, a, n, n, 3, o, stride, r, st)
    refused(capi.EINVAL, "n_in is negative", entry, sp._h, a, n, -1, 2, o, stride, r, st)
    refused(capi.EINVAL, "n_streams is negative", entry, sp._h, a, n, n, -1, o, stride, r, st)
    refused(capi.EINVAL, "in is null", entry, sp._h, None, n, n, 2, o, stride, r, st)
    refused(capi.EINVAL, "out is null", entry, sp._h, a, n, n, 2, None, stride, r, st)
    refused(capi.EINVAL, "in_stride is below n_in", entry, sp._h, a, n - 1, n, 2, o, stride, r, st)
    refused(capi.EINVAL, "out_stride is below n_rows nfft", entry, sp._h, a, n, n, 2, o, stride - 1, r, st)  # before any launch
    refused(capi.EINVAL, "out_stride is below n_rows nfft", entry, sp._h, a, n, n, 1, o, stride - 1, r, st)
    refused(capi.EINVAL, "in must be 8-byte aligned", entry, sp._h, a + 4, n, n, 2, o, stride, r, st)
    refused(capi.EINVAL, "out must be 4-byte aligned", entry, sp._h, a, n, n, 2, o + 2, stride, r, st)
    assert rows.value == -7
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()  # no refused call wrote anything
    # the host entry makes the same checks
    host_in, host_out = np.stack(xs), np.zeros((2, n_rows, nfft), np.float32)
    host = lib.dvbs2_spectrum_process
    hi, ho = host_in.ctypes.data, host_out.ctypes.data
    refused(capi.ESIZE, "n_in exceeds max_samples", host, sp._h, hi, n + 1, n + 1, 2, ho, stride, r)
    refused(capi.ESIZE, "n_streams exceeds max_streams", host, sp._h, hi, n, n, 3, ho, stride, r)
    refused(capi.EINVAL, "in is null", host, sp._h, None, n, n, 2, ho, stride, r)
    refused(capi.EINVAL, "out is null", host, sp._h, hi, n, n, 2, None, stride, r)
    refused(capi.EINVAL, "in_stride is below n_in", host, sp._h, hi, n - 1, n, 2, ho, stride, r)
    refused(capi.EINVAL, "out_stride is below n_rows nfft", host, sp._h, hi, n, n, 2, ho, stride - 1, r)
    assert (host_out == 0).all() and rows.value == -7
    # the handle holds no state: the good call behind the refusals gives what it gives on a fresh handle
    got = run_on_device(sp, xs)
    for i in range(2):
        same(got[i], SM.rows32(xs[i], nfft, hop, avg, hann(nfft), table(nfft), True), f"behind the refusals, stream {i}")
    sp.close()


# ------------------------------------------------------------------ 5. closed loop: carriers nobody told the receiver about
PLSC, ND, LEAD = L.PLSC, 4, 2001
SEQ = [PLSC, PLSC, L.DUMMY, PLSC, PLSC]
SPS, ROLLOFF, RRC_DELAY = 8, 0.2, 5
OFFSETS = (-0.7531, 0.7519)  # in symbol rates: off the bin centres of a 1024-point spectrum at 8 samples per symbol
ES_N0_DB, SCALE = 10.0, 1.0 / 37.0


@functools.lru_cache(maxsize=None)
def capture():
    """As tests/test_ddc_gpu.capture(): two carriers of short QPSK 1/4 frames with different payloads, shaped at 8 samples per symbol,
    moved to OFFSETS symbol rates and added; noise at Es/N0 = ES_N0_DB for the power of one carrier; all of it scaled by SCALE.
    Returns (the encoders' inputs [2], the samples on the device, their number, symbols per carrier)."""
    import torch
    st = stream()
    rx = pulse_taps(SPS, ROLLOFF, RRC_DELAY, 0.0, 1.0)
    tx = pulse_taps(SPS, ROLLOFF, RRC_DELAY).astype(np.float64)
    tx = (tx / np.convolve(tx, rx.astype(np.float64))[2 * SPS * RRC_DELAY]).astype(np.float32)
    d_sum, sent, power = None, [], []
    for k, off in enumerate(OFFSETS):
        sent_k, d_x, n, n_all, _ = L.transmit_symbols(SEQ, ND, L.GOLD, LEAD, seed=5000 + k, flush=256)
        sent.append(sent_k)
        ns = n_all * SPS
        ps = PulseShaper(SPS, taps=tx, max_symbols=n_all)
        d_y = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
        ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), ns, st)
        power.append(float((d_y[:n * SPS] ** 2).sum(dim=1).mean().item()))
        rot = Rotator(2 * np.pi * off / SPS)
        rot.work_device(d_y.data_ptr(), ns, d_y.data_ptr(), st)
        if d_sum is None:
            d_sum = torch.zeros_like(d_y)
        d_sum += d_y
        torch.cuda.synchronize()
        rot.close()
        ps.close()
    noise = Awgn(seed=78, sigma=awgn_sigma(ES_N0_DB, es=power[0], sps=SPS), max_samples=ns)
    noise.work_device(d_sum.data_ptr(), ns, ns, 1, d_sum.data_ptr(), ns, first_index=0, stream=st)
    d_sum *= SCALE
    torch.cuda.synchronize()
    noise.close()
    return sent, d_sum, ns, n_all


def receive(d_y, ns, n_syms, what):
    """d_y: ns samples of one channel at 2 per symbol on the device. AGC, timing recovery (cubic), frame search; a first PlCoarse pass
    over the frame records behind the lead gives the residual offset f, Rotator(-2 pi f) takes it off the symbols; then the decode
    tail of tests/loopback.py. Returns (messages, which encoder frame each carries, f in cycles per symbol)."""
    import torch
    st = stream()
    reference = float(torch.linalg.vector_norm(d_y[:2 * LEAD], dim=1).mean().item()) / SCALE
    agc = Agc(rate=0.05, reference=reference, gain=1.0, max_gain=65536.0, max_samples=ns)
    d_g = torch.zeros_like(d_y)
    agc.work_device(d_y.data_ptr(), ns, ns, 1, d_g.data_ptr(), ns, 0, 0, st)
    rx = L.timing_and_frames(d_g, ns, 2, ROLLOFF, SymbolSync.CUBIC, n_syms, tol=24)
    recs = rx.recs
    behind = np.nonzero(recs["sof_index"] >= LEAD)[0]
    assert rx.state == capi.PLSYNC_LOCKED and recs["plsc"][behind].tolist() == SEQ, (what, recs["plsc"].tolist())
    # One window over the data frames' records behind the lead, with the known PLSC: the estimate over all 90 header symbols of each
    # comes with the last. The front end's fine estimate between pilot blocks takes 1 / (2 * 1476) = 3.4e-4 cycles per symbol, which
    # the 26 symbols of the SOF form do not reach at this Es/N0.
    data_recs = [int(i) for i in behind if recs["plsc"][i] == PLSC]
    count = len(data_recs)
    d_sel = rx.d_rec.view(-1, 16)[torch.tensor(data_recs, device="cuda")].contiguous()
    pc = PlCoarse(count, PLSC, max_frames=64)
    d_f = torch.zeros(count, dtype=torch.float32, device="cuda")
    pc.work_records_device(rx.d_sym.data_ptr(), rx.nsym, 0, d_sel.data_ptr(), count, d_f.data_ptr(), 0, 0, st)
    torch.cuda.synchronize()
    f = float(d_f.cpu().numpy()[-1])
    pc.close()
    rot = Rotator(-2.0 * np.pi * f)
    rot.work_device(rx.d_sym.data_ptr(), rx.nsym, rx.d_sym.data_ptr(), st)
    torch.cuda.synchronize()
    rot.close()
    got = L.decode_frames(rx, PLSC, L.GOLD, 10 ** (-ES_N0_DB / 10), first_sof=LEAD)
    assert len(got.locked) >= ND - 1, what
    rx.sync.close()
    agc.close()
    return got.msg, got.data_index, f


def test_closed_loop_with_found_carriers():
    """Spectrum(1024, hop 512, avg 0, Hann, shifted) over the capture on the device; spectrum_carriers with defaults finds exactly two
    carriers, the centres within 0.01 symbol rates and the symbol rates within 2 %. From each record alone: the decimation
    round(1 / bandwidth / 2), the channel filter pulse_taps(round(1 / bandwidth), 0.2, 5, 0, 1) and set_channel(c, -2 pi centre). Each
    channel returns its own encoder's input bytes and not the other's."""
    import torch
    sent, d_wide, ns, n_all = capture()
    sp = Spectrum(1024, 512, 0, "hann", True, max_samples=ns)
    d_row = torch.zeros(1024, dtype=torch.float32, device="cuda")
    assert sp.work_device(d_wide.data_ptr(), ns, ns, 1, d_row.data_ptr(), 1024, stream()) == 1
    torch.cuda.synchronize()
    sp.close()
    row = d_row.cpu().numpy()
    recs, n_found = spectrum_carriers(row, True)
    print(f"found {n_found}: " + "; ".join(f"centre {c['centre'] * SPS:+.5f} symbol rates, {1 / c['bandwidth']:.4f} samples per symbol, "
                                          f"level / floor {c['level'] / c['floor']:.2f}" for c in recs))
    assert n_found == 2
    for c, off in zip(recs, OFFSETS):
        assert abs(c["centre"] * SPS - off) <= 0.01 and abs(c["bandwidth"] * SPS - 1) <= 0.02, (c, off)
    decims = {int(round(1 / c["bandwidth"] / 2)) for c in recs}
    spss = {int(round(1 / c["bandwidth"])) for c in recs}
    assert decims == {SPS // 2} and spss == {SPS}  # (one handle serves both: the two carriers have one symbol rate)
    dd = Ddc(decims.pop(), pulse_taps(spss.pop(), ROLLOFF, RRC_DELAY, 0.0, 1.0), max_channels=2, max_samples=ns)
    for ch, c in enumerate(recs):
        dd.set_channel(ch, -2.0 * np.pi * float(c["centre"]))
    n_out = dd.produce(ns)
    d_ch = torch.zeros((2, n_out, 2), dtype=torch.float32, device="cuda")
    assert dd.work_device(d_wide.data_ptr(), ns, ns, 1, 2, d_ch.data_ptr(), n_out, stream()) == n_out
    torch.cuda.synchronize()
    for ch in range(2):
        msg, data_index, f = receive(d_ch[ch], n_out, n_all, f"channel {ch}")
        left = OFFSETS[ch] - float(recs[ch]["centre"]) * SPS  # what the finder left, in cycles per symbol
        print(f"channel {ch}: residual offset estimated {f:+.5f}, true {left:+.5f} cycles per symbol")
        assert np.array_equal(msg, sent[ch][data_index]), ch  # the encoder's input bytes
        assert not np.array_equal(msg, sent[ch ^ 1][data_index])
    dd.close()
