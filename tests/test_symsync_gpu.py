"""Symbol timing recovery on the device (dvbs2_symsync_*) against restatement (b) of tests/symsync_model.py, bit for bit: symbols,
strobe indices, the mu trace, n_out, consumed and the final state, for the four interpolators at 2 and 4 samples per symbol, loop
closed and open; the same bits however a stream is cut into calls or batched with others; the stop status; the pipeline Rotator ->
SymbolSync -> PlSync -> PlCoarse -> PlFrontEnd -> FecChain on samples with a carrier and a timing offset; and the C++ host mirror.
Every closed-loop input is vouched for by tests/test_symsync_model.py. The model runs on the bank the library designed
(symsync_taps), so the comparison does not depend on libm."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import plcoarse_model as K
import plframe_model as M
import plsync_model as P
import symsync_model as S
from dvbs2rx_amd import Rotator, SymbolSync, capi, symsync_taps

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize % 8 else np.uint64)


def run_batch(ss, streams, max_out=None):
    """one work_device() over a batch; returns per stream (symbols, strobe indices, mu, consumed, status)"""
    import torch
    ns = len(streams)
    stride = max(max(x.size for x in streams), 1)
    cap = stride if max_out is None else max_out
    buf = np.zeros((ns, stride), np.complex64)
    for i, x in enumerate(streams):
        buf[i, :x.size] = x
    d_in = dev(buf)
    ocap = max(cap, 1)
    d_out = torch.full((ns, ocap * 2), -7.0, dtype=torch.float32, device="cuda")
    d_idx = torch.full((ns, ocap), -7, dtype=torch.int64, device="cuda")
    d_mu = torch.full((ns, ocap), -7.0, dtype=torch.float64, device="cuda")
    ss.work_device(d_in.data_ptr(), stride, [x.size for x in streams], d_out.data_ptr(), ocap, cap, d_idx.data_ptr(), d_mu.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    n_out, consumed, status = ss.finish()
    out, idx, mu = d_out.cpu().numpy().view(np.complex64), d_idx.cpu().numpy(), d_mu.cpu().numpy()
    res = []
    for i in range(ns):
        k = int(n_out[i])
        assert (out[i, k:].real == -7.0).all() and (idx[i, k:] == -7).all()  # nothing written past n_out
        res.append((out[i, :k].copy(), idx[i, :k].copy(), mu[i, :k].copy(), int(consumed[i]), int(status[i])))
    return res


def same(got, want, what):
    assert got[3:] == want[3:], (what, got[3:], want[3:])
    assert got[0].size == want[0].size, (what, got[0].size, want[0].size)
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits(got[2]), bits(want[2])), what
    assert np.array_equal(bits(got[0]), bits(want[0])), what


def same_state(ss, i, m, what):
    g, w = ss.state(i), m.state()
    for k in ("vi", "cnt", "mu"):
        assert np.float64(g[k]).view(np.uint64) == np.float64(w[k]).view(np.uint64), (what, k, g[k], w[k])
    assert bits(np.complex64(g["last_xi"]).reshape(1)).tolist() == bits(np.complex64(w["last_xi"]).reshape(1)).tolist(), what
    assert (g["jump"], g["init"], g["status"], g["n_read"]) == (w["jump"], w["init"], w["status"], w["n_read"]), what


@functools.lru_cache(maxsize=None)
def bank_of(sps, rolloff, rrc_delay, n_subfilt):
    return symsync_taps(sps, rolloff, rrc_delay, n_subfilt)


def model(cfg):
    return S.SymSync(bank=bank_of(cfg["sps"], cfg["rolloff"], cfg["rrc_delay"], cfg["n_subfilt"]), **cfg)


# ------------------------------------------------------------------ 1. bit for bit against the restatement
def test_matlab_vectors_and_open_loop():
    for v, x, want in S.kat_vectors():
        cfg = S.kat_cfg(v)
        ss, m = SymbolSync(**cfg), model(cfg)
        got = run_batch(ss, [x])[0]
        same(got, m.work(x), v["name"])
        same_state(ss, 0, m, v["name"])
        d = got[0].astype(np.complex128) - want  # the reference's own tolerance, on the device's output
        assert (np.round(d.real, S.KAT["places"]) == 0).all() and (np.round(d.imag, S.KAT["places"]) == 0).all()
        ss.close()
    # the reference's open-loop case (linear, sps 2), and the same symbols at sps 4; the Farrow forms return the sample before
    # the basepoint at mu = 0 (tests/test_symsync_model.py), so they see the symbols one sample later
    x2, syms = S.open_loop_input()
    x4 = np.zeros(syms.size * 4, np.complex64)
    x4[::4] = syms
    for sps, x in ((2, x2), (4, x4)):
        for interp in (1, 2, 3):
            cfg = dict(sps=sps, loop_bw=0.01, damping=0.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp_method=interp)
            xi = x if interp == 1 else np.roll(x, sps - 1)
            ss, m = SymbolSync(**cfg), model(cfg)
            got = run_batch(ss, [xi])[0]
            same(got, m.work(xi), f"open loop sps {sps} interp {interp}")
            same_state(ss, 0, m, f"open loop sps {sps} interp {interp}")
            want = syms[1:] if interp == 1 else syms[:6]
            assert np.array_equal(got[0], want) and (got[2] == 0).all()  # the reference's assertListEqual
            assert sps != 2 or got[3] == x.size
            ss.close()


@pytest.mark.parametrize("name", [c[0] for c in S.CLOSED_SETS])
def test_closed_loop_sets(name):
    cfg, x = S.closed_set(name)
    ss, m = SymbolSync(**cfg), model(cfg)
    got = run_batch(ss, [x])[0]
    want = m.work(x)
    same(got, want, name)
    same_state(ss, 0, m, name)
    assert want[4] == 0 and want[0].size > 1000 and len(set(np.diff(want[1]).tolist())) >= 2
    # open loop on the same samples, every interpolator
    c0 = dict(cfg, damping=0.0)
    ss0, m0 = SymbolSync(**c0), model(c0)
    same(run_batch(ss0, [x])[0], m0.work(x), name + " open loop")
    same_state(ss0, 0, m0, name + " open loop")
    ss.close()
    ss0.close()


def test_host_entry_and_caller_taps():
    cfg, x = S.closed_set("poly-sps2")
    ss, m = SymbolSync(**cfg), model(cfg)
    same(ss.work(x), m.work(x), "host entry")
    ss.close()
    rng = np.random.default_rng(4)
    mine = (bank_of(2, 0.2, 5, 128) * rng.uniform(0.9, 1.1, (128, 21))).astype(np.float32)  # a bank that is not the library's
    ss, m = SymbolSync(taps=mine, **cfg), S.SymSync(bank=mine, **cfg)
    same(ss.work(x), m.work(x), "caller's taps")
    ss.close()


# ------------------------------------------------------------------ 2. cut invariance
def in_pieces(ss, x, piece, max_out=None):
    """present `piece` new samples per call behind whatever the last call left unconsumed, as a scheduler would"""
    pos, end, outs, calls = 0, 0, [], 0
    while True:
        end = min(x.size, end + piece)
        o, i, mu, consumed, status = run_batch(ss, [x[pos:end]], max_out)[0]
        assert status == 0 and consumed <= end - pos
        outs.append((o, i, mu))
        pos += consumed
        calls += 1
        if end == x.size and consumed == 0 and (max_out is None or o.size < max_out):
            break
    return tuple(np.concatenate([p[k] for p in outs]) for k in range(3)), pos, calls


@pytest.mark.parametrize("name", ["poly-sps4", "lin-sps4", "cub-sps2", "poly-sps2", "poly-sps4-short"])
def test_cuts_give_the_same_bits(name):
    cfg, x = S.closed_set(name.replace("-short", ""))
    if name in ("cub-sps2", "poly-sps2", "poly-sps4-short"):
        x = x[:700]  # the one-sample pieces: one launch per sample; polyphase histories of 21 and 42 samples are cut at every position
    ss = SymbolSync(**cfg)
    whole = run_batch(ss, [x])[0]
    st_whole = ss.state(0)
    for piece, max_out in ((1, None), (7, None), (4096, None), (512, 37)) if x.size <= 700 else ((7, None), (4096, None), (512, 37)):
        ss.reset()
        (o, i, mu), pos, calls = in_pieces(ss, x, piece, max_out)
        what = f"{name} pieces of {piece} max_out {max_out}: {calls} calls"
        assert pos == whole[3], what
        assert np.array_equal(bits(o), bits(whole[0])) and np.array_equal(i, whole[1]) and np.array_equal(bits(mu), bits(whole[2])), what
        st = ss.state(0)
        assert all(np.float64(st[k]).view(np.uint64) == np.float64(st_whole[k]).view(np.uint64) for k in ("vi", "cnt", "mu")) and \
            st["n_read"] == st_whole["n_read"] and st["jump"] == st_whole["jump"], what
    ss.reset()  # reset restores the initial behaviour
    again = run_batch(ss, [x])[0]
    same(again, whole, name + " after reset")
    ss.close()


# ------------------------------------------------------------------ 3. batch invariance
@pytest.mark.parametrize("interp", [0, 1])
def test_a_batch_gives_each_stream_the_bits_of_that_stream_alone(interp):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nstreams = n_cu + 45  # more streams than CUs
    cfg, x = S.closed_set("poly-sps2" if interp == 0 else "lin-sps2")
    rng = np.random.default_rng(31)
    lens = rng.integers(0, x.size, nstreams)
    lens[:4] = (0, 1, 2, x.size)
    offs = [int(rng.integers(0, x.size - n + 1)) for n in lens]
    streams = [x[o:o + n] for o, n in zip(offs, lens)]
    ss = SymbolSync(max_streams=nstreams, **cfg)
    got = run_batch(ss, streams)
    solo = SymbolSync(**cfg)
    for i in range(nstreams):  # every stream: symbols, indices, mu, consumed and status of that stream run alone (S = 1)
        solo.reset()
        same(got[i], run_batch(solo, [streams[i]])[0], f"stream {i} of {nstreams}, {lens[i]} samples")
        assert got[i][4] == 0
    for i in list(range(6)) + list(range(6, nstreams, 16)) + [nstreams - 1]:
        m = model(cfg)
        same(got[i], m.work(streams[i]), f"stream {i} against the model")
        same_state(ss, i, m, f"stream {i}")
    assert got[0][3:] == (0, 0) and got[1][3:] == (0, 0) and got[2][3] == 2  # nothing to start on; two samples start the loop
    ss.close()
    solo.close()


# ------------------------------------------------------------------ 4. stop status
def test_stopped_streams_stop_alone():
    x = S.qpsk_stream(**S.STOP_STREAM)[0]
    good = S.closed_set("lin-sps2")[1][:x.size]
    nan = good.copy()
    nan[301] = np.nan
    cfg = S.STOP_CFG
    ss = SymbolSync(max_streams=3, **cfg)
    got = run_batch(ss, [x, nan, good[:400]])
    m = [S.SymSync(**cfg) for _ in range(3)]
    want = [m[0].work(x), m[1].work(nan), m[2].work(good[:400])]
    assert want[0][4] == 1 and want[1][4] == 2 and want[2][4] == 0, [w[4] for w in want]
    print("stopped after", [w[0].size for w in want], "symbols, consumed", [w[3] for w in want], "status", [w[4] for w in want])
    for i in (0, 2):
        same(got[i], want[i], f"stream {i}")
    # the NaN stream: every symbol before the stop bit for bit, the last one NaN, and the stop where the model names it
    g, w = got[1], want[1]
    assert g[3:] == w[3:] and g[0].size == w[0].size and np.array_equal(g[1], w[1]) and np.array_equal(bits(g[2]), bits(w[2]))
    assert np.array_equal(bits(g[0][:-1]), bits(w[0][:-1])) and np.isnan(g[0][-1]) and np.isnan(w[0][-1])
    # later calls on stopped streams return at once; the third stream goes on, untouched
    rest = [x[want[0][3]:], nan[want[1][3]:], good[want[2][3]:]]
    got2 = run_batch(ss, rest)
    assert got2[0][3:] == (0, 1) and got2[0][0].size == 0 and got2[1][3:] == (0, 2) and got2[1][0].size == 0
    same(got2[2], m[2].work(rest[2]), "the running stream, second call")
    same_state(ss, 2, m[2], "the running stream")
    # reset restores the initial behaviour, on the streams that had stopped too
    ss.reset()
    again = run_batch(ss, [good[:400], x, good[:400]])
    fresh = [S.SymSync(**cfg) for _ in range(3)]
    for i, inp in enumerate((good[:400], x, good[:400])):
        same(again[i], fresh[i].work(inp), f"after reset, stream {i}")
        same_state(ss, i, fresh[i], f"after reset, stream {i}")
    assert again[0][4] == 0 and again[1][4] == 1 and again[2][4] == 0
    ss.close()


# ------------------------------------------------------------------ 5. the pipeline, from samples
E2E_TAU, E2E_SPS = 0.37, 2


def shaped_samples(x):
    """the symbol stream of plcoarse_model.e2e_stream (carrier offset and noise included) as RRC-shaped samples at 2 per symbol,
    with a timing offset of E2E_TAU symbols; the carrier offset per SAMPLE is half the one per symbol"""
    delay = 8
    n = (x.size - 1) * E2E_SPS
    t = np.arange(n) / E2E_SPS + E2E_TAU
    k0 = np.floor(t).astype(int)
    y = np.zeros(n, np.complex128)
    xs = x.astype(np.complex128) * np.exp(-1j * M.PI2 * K.E2E_FOFFSET * np.arange(x.size))  # the symbols without their rotation ...
    for d in range(-delay, delay + 1):
        k = k0 + d
        ok = (k >= 0) & (k < x.size)
        y[ok] += xs[k[ok]] * S.rrc(t[ok] - k[ok], 0.2)
    g = np.arange(-delay * E2E_SPS, delay * E2E_SPS + 1) / E2E_SPS
    y /= np.sum(S.rrc(g, 0.2) ** 2) / np.sum(S.rrc(g, 0.2))
    return (y * np.exp(1j * M.PI2 * K.E2E_FOFFSET / E2E_SPS * np.arange(n))).astype(np.complex64)  # ... and the carrier on the samples


def test_pipeline_from_samples_to_bbframes():
    import torch
    x, sofs, sent, plsc = K.e2e_stream()
    y = shaped_samples(x)
    e = P.E2E["e2e-qpsk"]
    d_y = dev(y)
    # Rotator on samples (the offset known here, as after a first coarse estimate), then timing recovery and matched filter
    rot = Rotator(-M.PI2 * K.E2E_FOFFSET / E2E_SPS)
    rot.work_device(d_y.data_ptr(), y.size, d_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rx = L.timing_and_frames(d_y, y.size, E2E_SPS, 0.2, 0, x.size, tol=12, plsc=plsc)
    assert rx.state == capi.PLSYNC_LOCKED and rx.nf == len(sofs)
    shift = set((rx.recs["sof_index"] - np.array(sofs)).tolist())
    assert len(shift) == 1 and abs(shift.pop()) <= 12  # one constant delay: the loop's start-up and the filter
    got = L.decode_frames(rx, plsc, P.E2E_GOLD, 10 ** (-K.E2E_ES_N0_DB / 10), descramble=False,
                          fec=dict(framesize=capi.FECFRAME_SHORT, rate=e["rate"], constellation=capi.MOD_QPSK))
    print(f"{rx.nsym} symbols from {y.size} samples, residual offsets {got.offsets}, coarse_corrected {got.corrected.tolist()}")
    assert len(got.locked) >= len(sofs) - 1
    assert got.corrected.all()
    assert np.array_equal(got.msg, sent[got.locked])  # the transmitted BBFRAMEs
    rx.sync.close()
    rot.close()


# ------------------------------------------------------------------ 6. the C++ host mirror
def test_host_mirror(tmp_path):
    libdir = os.path.join(T.ROOT, "gr-dvbs2rx_amd", "lib")
    exe = str(tmp_path / "symsync_host_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(T.ROOT, "tests", "symsync_host_main.cpp"), "-o", exe,
                           "-L" + libdir, "-ldvbs2_fec_hip", "-Wl,-rpath," + libdir])

    def run(x, cfg, chunk, tag_period):
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        x.tofile(fin)
        r = subprocess.run([exe, fin, fout] + [str(cfg[k]) for k in ("sps", "loop_bw", "damping", "rolloff", "rrc_delay", "n_subfilt", "interp_method")] +
                           [str(chunk), str(tag_period)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        tags = [int(t) for t in r.stdout.split("tags")[1].split()]
        return np.fromfile(fout, np.complex64), tags, r.stdout

    # the reference's tag test: open loop, tags every 2 sps samples land at 0, 1, 3, 5, ...
    t = S.KAT["tags"]
    rng = np.random.default_rng(1)
    a = (((1 - 2.0 * rng.integers(0, 2, t["nsyms"])) + 1j * (1 - 2.0 * rng.integers(0, 2, t["nsyms"]))) * np.sqrt(0.5)).astype(np.complex64)
    x = np.zeros(t["nsyms"] * t["sps"], np.complex64)
    x[::t["sps"]] = a
    cfg = dict(sps=2, loop_bw=0.01, damping=0.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp_method=1)
    want_tags = [0] + list(range(1, t["nsyms"] - 1, 2))
    for chunk in (x.size, 9):  # one call; many calls, tags pending between them
        out, tags, log = run(x, cfg, chunk, t["tag_period"])
        assert np.array_equal(out, a[1:1 + out.size]) and out.size == t["nsyms"] - 1, log
        assert tags == want_tags[:len(tags)] and len(tags) >= len(want_tags) - 1, log
    # closed loop, polyphase, in calls of 1000 samples: the symbols of the model, tags placed as the model places them
    cfg, x = S.closed_set("poly-sps2")
    m = model(cfg)
    o, idx, mu, consumed, status = m.work(x)
    out, tags, log = run(x, cfg, 1000, 64)
    assert np.array_equal(bits(out), bits(o)) and f"consumed {consumed} produced {o.size} history {m.H}" in log, log
    placed, pending = S.map_tag_offsets(list(range(0, consumed, 64)), 0, idx + m.H, 0, m.H + m.D - 1)
    assert tags == placed, log
