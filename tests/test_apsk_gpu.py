"""GPU: the 16APSK / 32APSK soft demapper (DVB-S2 MODCODs 18-28) -- bit for bit against the float32 restatement of
tests/apsk_model.py and under its float64 bound, the SNR estimates against the float64 model, and end to end: encoded BBFRAMEs
through mapper and AWGN back through FecChain, and from PLFRAMEs through the PL front end. The constellation tables are UNPINNED
(the reference has no APSK modulator or demapper; apsk_model.py holds an independent restatement of EN 302 307-1)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import apsk_model as A
import fec_testlib as T
import plframe_model as M
from dvbs2rx_amd import Demapper, FecChain, PlFrontEnd, apsk_points, capi, get_fec_info
from dvbs2rx_amd.blocks import rate_id

pytestmark = pytest.mark.gpu

SHORT, NORMAL = capi.FECFRAME_SHORT, capi.FECFRAME_NORMAL
# the four shapes: rows 4050 (no multiple of 4: odd columns are 2 bytes off a dword, the last quad holds 2 symbols), 16200, 3240, 12960
SHAPES = [("16apsk-short-2_3", capi.MOD_16APSK, SHORT, "C2_3", 4050), ("16apsk-normal-9_10", capi.MOD_16APSK, NORMAL, "C9_10", 16200),
          ("32apsk-short-3_4", capi.MOD_32APSK, SHORT, "C3_4", 3240), ("32apsk-normal-9_10", capi.MOD_32APSK, NORMAL, "C9_10", 12960)]
N0_FRAMES = np.array([0.2, 0.05, 0.01], np.float32)


@functools.lru_cache(maxsize=None)
def demap_case(constellation, rate, rows):
    """3 frames of point + noise at N0 = 0.2, 0.05, 0.01, with the symbols 0 and (1e3, -1e3) planted at both ends and in between;
    the restatement's LLRs for the per-frame N0 and for N0 = 0.01 on all frames. Computed once, never modified."""
    rng = np.random.default_rng(rows + constellation)
    p = A.points(constellation, rate)
    tx = p[rng.integers(0, len(p), (3, rows))]
    noise = np.sqrt(N0_FRAMES.astype(np.float64) / 2.0)[:, None] * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))
    syms = (tx + noise).astype(np.complex64)
    for f in range(3):
        syms[f, [0, rows - 2, 1000 + f]] = 0
        syms[f, [1, rows - 1, 2001 + f]] = 1e3 - 1e3j
    lib_pts = apsk_points(constellation, rate)
    per_frame = A.demap_f32(syms, N0_FRAMES, lib_pts)[0]
    one = A.demap_f32(syms, N0_FRAMES[2], lib_pts)[0]
    for a in (syms, per_frame, one):
        a.setflags(write=False)
    return syms, per_frame, one, p


@pytest.mark.parametrize("name,constellation,framesize,rate,rows", SHAPES, ids=[s[0] for s in SHAPES])
def test_demap_bit_for_bit(name, constellation, framesize, rate, rows):
    import torch
    syms, want_pf, want_one, p = demap_case(constellation, rate, rows)
    n_mod = A.N_MOD[constellation]
    dm = Demapper(framesize=framesize, rate=rate, constellation=constellation, max_frames=3)
    assert (dm.n_syms, dm.n_mod, dm.column_order, dm.n_llr) == (rows, n_mod, 0, rows * n_mod)
    sat = np.mean((want_pf[2] == 127) | (want_pf[2] == -128))
    print(f"{name}: saturated share at N0 0.01 {sat:.3f}")
    assert 0.05 < sat < 0.25  # the run covers saturation
    # against float64 with the near-half-integer rule (the planted far symbol enters D_max, so the bound is checked on the rest)
    keep = np.ones(rows, bool)
    keep[[0, 1, rows - 2, rows - 1, 1000, 1001, 1002, 2001, 2002, 2003]] = False
    sel = np.concatenate([np.flatnonzero(keep) + c * rows for c in range(n_mod)])
    A.check_vs_f64(want_pf[:, sel], syms[:, keep], N0_FRAMES, p, name + " restatement")
    # host entry
    assert np.array_equal(dm.work(syms, N0_FRAMES), want_pf)
    assert np.array_equal(dm.work(syms, N0_FRAMES[2]), want_one)
    # device entry, canaries in front of and behind the output
    pad = 256
    d_syms = torch.from_numpy(syms.view(np.float32).copy()).cuda()
    d_n0 = torch.from_numpy(N0_FRAMES.copy()).cuda()
    for n0_ptr, n0_count, want in ((d_n0.data_ptr(), 3, want_pf), (d_n0.data_ptr() + 8, 1, want_one)):
        d_out = torch.full((pad + 3 * dm.n_llr + pad,), 0x5A, dtype=torch.int8, device="cuda")
        dm.work_device(d_syms.data_ptr(), 3, n0_ptr, n0_count, d_out.data_ptr() + pad)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert (out[:pad] == 0x5A).all() and (out[-pad:] == 0x5A).all()
        got = out[pad:-pad].reshape(3, -1)
        A.check_vs_f64(got[:, sel], syms[:, keep], N0_FRAMES if n0_count == 3 else N0_FRAMES[2], p, name + " device")
        assert np.array_equal(got, want)
    # two frames of three: the third frame's bytes stay
    d_out = torch.full((3 * dm.n_llr,), 0x5A, dtype=torch.int8, device="cuda")
    dm.work_device(d_syms.data_ptr(), 2, d_n0.data_ptr(), 2, d_out.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().reshape(3, -1)
    assert np.array_equal(out[:2], want_pf[:2]) and (out[2] == 0x5A).all()
    dm.close()


def test_single_frame_handle_and_empty_calls():
    import torch
    name, constellation, framesize, rate, rows = SHAPES[0]
    syms, want_pf, _, _ = demap_case(constellation, rate, rows)
    dm = Demapper(framesize=framesize, rate=rate, constellation=constellation, max_frames=1)
    for f in range(3):
        assert np.array_equal(dm.work(syms[f:f + 1], N0_FRAMES[f]), want_pf[f:f + 1])
    lib = capi.lib
    assert lib.dvbs2_demap_soft_device(dm._h, None, 0, None, 1, None, None) == capi.OK
    assert lib.dvbs2_demap_soft(dm._h, None, 0, None, 1, None) == capi.OK
    assert lib.dvbs2_demap_estimate_snr(dm._h, None, 0, None) == capi.OK
    out = np.empty((2, dm.n_llr), np.int8)
    two = np.ascontiguousarray(syms[:2])
    assert lib.dvbs2_demap_soft(dm._h, two.ctypes.data, 2, N0_FRAMES.ctypes.data, 1, out.ctypes.data) == capi.ESIZE
    dm.close()
    chain = FecChain(framesize=framesize, rate=rate, constellation=constellation, group_size=4, max_frames=1, max_trials=5)
    assert chain.n_syms == rows
    d_msg = torch.zeros(chain.msg_bytes, dtype=torch.uint8, device="cuda")
    chain.work_device(0, 0, 0, 1, d_msg.data_ptr())
    msg, _, _ = chain.work(np.zeros((0, rows), np.complex64), 0.1)
    assert msg.shape == (0, chain.msg_bytes)
    chain.close()


def test_rejected_combinations():
    h = C.c_void_p()
    lib = capi.lib
    bad = [(capi.MOD_16APSK, NORMAL, "C1_2", b"rate"), (capi.MOD_16APSK, NORMAL, "C3_5", b"rate"), (capi.MOD_16APSK, NORMAL, "C7_8", b"rate"),
           (capi.MOD_32APSK, NORMAL, "C2_3", b"rate"), (capi.MOD_32APSK, SHORT, "C7_8", b"rate"), (capi.MOD_16APSK, NORMAL, "C26_45", b"rate"),
           (capi.MOD_16APSK, SHORT, "C9_10", b"rate"), (capi.MOD_32APSK, SHORT, "C9_10", b"rate"),
           (capi.MOD_16APSK, capi.FECFRAME_MEDIUM, "C3_4", b"frame size"),
           (3, NORMAL, "C3_4", b"Unsupported constellation"), (5, NORMAL, "C3_4", b"Unsupported constellation"),
           (7, NORMAL, "C3_4", b"Unsupported constellation"), (9, NORMAL, "C3_4", b"Unsupported constellation")]
    for constellation, framesize, rate, text in bad:
        assert lib.dvbs2_demap_create(C.byref(h), framesize, rate_id(rate), constellation, 4, 0) == capi.EINVAL and not h.value
        assert text in lib.dvbs2_last_error(), (constellation, rate, lib.dvbs2_last_error())
        assert lib.dvbs2_chain_create(C.byref(h), capi.STANDARD_DVBS2, framesize, rate_id(rate), constellation, 4, 4, 0) == capi.EINVAL and not h.value
    for constellation, rates in ((capi.MOD_16APSK, A.GAMMA_16), (capi.MOD_32APSK, A.GAMMA_32)):
        for rate in rates:
            for framesize in (NORMAL,) if rate == "C9_10" else (NORMAL, SHORT):
                dm = Demapper(framesize=framesize, rate=rate, constellation=constellation, max_frames=1)
                assert dm.n_mod == A.N_MOD[constellation] and dm.column_order == 0
                dm.close()


# ------------------------------------------------------------------ SNR estimates
@pytest.mark.parametrize("name,constellation,framesize,rate,rows", SHAPES[:1] + SHAPES[2:], ids=[s[0] for s in SHAPES[:1] + SHAPES[2:]])
def test_snr_estimates(name, constellation, framesize, rate, rows):
    import torch
    sigma = np.array([0.05, 0.2, 0.4])
    rng = np.random.default_rng(rows)
    p = A.points(constellation, rate)
    n_mod = A.N_MOD[constellation]
    bits = rng.integers(0, 2, (3, rows * n_mod), dtype=np.uint8)
    tx = A.map_bits(bits, p)
    syms = (tx + sigma[:, None] * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))).astype(np.complex64)
    llr = np.where(bits == 1, rng.integers(-128, 0, bits.shape), rng.integers(0, 128, bits.shape)).astype(np.int8)  # 0 counts as bit 0
    dm = Demapper(framesize=framesize, rate=rate, constellation=constellation, max_frames=3)
    pre, want_pre = dm.estimate_snr(syms), A.snr_f64(syms, p)
    post, want_post = dm.refine_snr(syms, llr), A.snr_f64(syms, p, llr)
    print(f"{name}: estimate_snr {pre} (model {want_pre}), refine_snr {post} (model {want_post}), 1 / (2 sigma^2) {1 / (2 * sigma ** 2)}")
    assert np.allclose(pre, want_pre, rtol=2e-4, atol=0)
    assert np.allclose(post, want_post, rtol=2e-4, atol=0)
    assert np.allclose(post, 1.0 / (2.0 * sigma ** 2), rtol=0.05, atol=0)
    # device entries: the same values
    d_syms = torch.from_numpy(syms.view(np.float32).copy()).cuda()
    d_llr = torch.from_numpy(llr).cuda()
    d_snr = torch.zeros(6, dtype=torch.float32, device="cuda")
    capi.check(capi.lib.dvbs2_demap_estimate_snr_device(dm._h, d_syms.data_ptr(), 3, d_snr.data_ptr(), None))
    capi.check(capi.lib.dvbs2_demap_refine_snr_device(dm._h, d_syms.data_ptr(), d_llr.data_ptr(), 3, d_snr.data_ptr() + 12, None))
    torch.cuda.synchronize()
    assert np.array_equal(d_snr.cpu().numpy(), np.concatenate([pre, post]))
    dm.close()


# ------------------------------------------------------------------ end to end
def encoded_frames(framesize, rate, nf, seed):
    fi = get_fec_info(capi.STANDARD_DVBS2, framesize, rate)
    m, prim = T.BCH_FIELDS[framesize]
    ob = T.OracleBch(m, prim, fi["bch_t"], fi["bch_n"])
    rng = np.random.default_rng(seed)
    sent = rng.integers(0, 256, (nf, fi["bch_k"] // 8), dtype=np.uint8)
    cw = T.ldpc_encode(fi["table"], np.unpackbits(ob.encode_bytes(sent), axis=1))
    return sent, cw, rng


@pytest.mark.parametrize("constellation,rate,es_n0_db", [(capi.MOD_16APSK, "C2_3", 12.0), (capi.MOD_32APSK, "C3_4", 15.7)], ids=["16apsk-2_3", "32apsk-3_4"])
def test_end_to_end_chain(constellation, rate, es_n0_db):
    """32 short frames 3 dB above the quasi-error-free point of EN 302 307-1 table 13: BCH + LDPC encoders, column interleaver,
    the model's mapper, AWGN, then FecChain from symbols on the device entry and from host buffers. Every message comes back,
    the decoder had errors to correct, and the chain equals demapper -> LLR chain byte for byte."""
    import torch
    nf = 32
    sent, cw, rng = encoded_frames(SHORT, rate, nf, 77 + constellation)
    p = A.points(constellation, rate)
    n0 = np.float32(10.0 ** (-es_n0_db / 10.0))
    tx = A.map_bits(cw, p)
    syms = (tx + np.sqrt(float(n0) / 2.0) * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))).astype(np.complex64)
    chain = FecChain(framesize=SHORT, rate=rate, constellation=constellation, group_size=32, max_frames=nf, max_trials=50)
    assert chain.n_syms == syms.shape[1]
    d_syms = torch.from_numpy(syms.view(np.float32).copy()).cuda()
    d_n0 = torch.full((1,), float(n0), dtype=torch.float32, device="cuda")
    d_msg = torch.zeros((nf, chain.msg_bytes), dtype=torch.uint8, device="cuda")
    d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_corr = torch.zeros(nf, dtype=torch.int32, device="cuda")
    chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr())
    torch.cuda.synchronize()
    msg_dev, ret_dev, corr_dev = d_msg.cpu().numpy(), d_ret.cpu().numpy(), d_corr.cpu().numpy()
    assert (ret_dev >= 0).all() and (corr_dev >= 0).all()
    assert np.array_equal(msg_dev, sent)
    msg_host, ret_host, corr_host = chain.work(syms, n0)  # dvbs2_chain_decode: the chunked host pipeline
    assert np.array_equal(msg_host, sent) and (ret_host >= 0).all() and (corr_host >= 0).all()
    assert chain.fallback_rounds == 0
    # the demapper's hard decisions are wrong in places: the decoder did the work
    dm = Demapper(framesize=SHORT, rate=rate, constellation=constellation, max_frames=nf)
    d_llr = torch.zeros((nf, dm.n_llr), dtype=torch.int8, device="cuda")
    dm.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_llr.data_ptr())
    torch.cuda.synchronize()
    llr = d_llr.cpu().numpy()
    assert np.array_equal(llr, A.demap_f32(syms, n0, apsk_points(constellation, rate))[0])
    ber = np.mean((llr < 0).astype(np.uint8) != cw)
    print(f"Es/N0 {es_n0_db} dB: hard-decision bit error rate before the decoder {ber:.4f}, LDPC ret {ret_dev}, BCH corrections {corr_dev.sum()}")
    assert 1e-3 < ber < 0.1
    # the same bytes from demapper -> chain from LLRs
    ll = FecChain(framesize=SHORT, rate=rate, group_size=32, max_frames=nf, max_trials=50, from_llr=True)
    d_msg2 = torch.zeros_like(d_msg)
    d_ret2, d_corr2 = torch.zeros_like(d_ret), torch.zeros_like(d_corr)
    ll.work_llr_device(d_llr.data_ptr(), nf, d_msg2.data_ptr(), d_ret2.data_ptr(), d_corr2.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_msg2.cpu().numpy(), msg_dev)
    assert np.array_equal(d_ret2.cpu().numpy(), ret_dev) and np.array_equal(d_corr2.cpu().numpy(), corr_dev)
    for o in (chain, dm, ll):
        o.close()


def test_plframe_to_bbframe_16apsk():
    """MODCOD 18 (16APSK 2/3), short frames, pilots: 8 PLFRAMEs with a constant phase and a fine frequency offset through
    dvbs2_plframe_process and the 16APSK chain."""
    nf, gold, es_n0_db = 8, 5, 12.0
    plsc = (18 << 2) | (1 << 1) | 1
    sent, cw, rng = encoded_frames(SHORT, "C2_3", nf, 18)
    syms = A.map_bits(cw, A.points(capi.MOD_16APSK, "C2_3"))
    info = M.pls_parse(plsc)
    assert syms.shape[1] == info["xfecframe_len"] == 4050 and info["n_slots"] == 45
    frames, _ = M.make_plframes(plsc, gold, nf, rng, es_n0_db=es_n0_db, phase=2.1, foffset=2e-4, data=syms)
    fe = PlFrontEnd(gold, plsc, max_frames=nf)
    xfec, est = fe.work(frames, np.ones(nf, np.int32))
    assert (est["plsc_decoded"] == plsc).all() and (est["fine_valid"] == 1).all()
    print(f"fine_foffset {est['fine_foffset']}")
    chain = FecChain(framesize=SHORT, rate="C2_3", constellation=capi.MOD_16APSK, group_size=4, max_frames=nf, max_trials=50)
    msg, ret, corr = chain.work(xfec, np.float32(10 ** (-es_n0_db / 10)))
    print(f"LDPC ret {ret}, BCH corrections {corr}")
    assert (ret >= 0).all() and (corr >= 0).all()
    assert np.array_equal(msg, sent)
    chain.close()
    fe.close()


# ------------------------------------------------------------------ the C++ host mirror
def test_host_mirror(tmp_path):
    libdir = os.path.join(T.ROOT, "gr-dvbs2rx_amd", "lib")
    exe = str(tmp_path / "apsk_host_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(T.ROOT, "tests", "apsk_host_main.cpp"), "-o", exe,
                           "-L" + libdir, "-ldvbs2_fec_hip", "-Wl,-rpath," + libdir])
    for name, constellation, framesize, rate, rows in (SHAPES[0], SHAPES[2]):
        syms, _, _, p = demap_case(constellation, rate, rows)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        syms.tofile(fin)
        r = subprocess.run([exe, fin, fout, str(framesize), rate, str(constellation), "20.0"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        n0 = np.float32(1.0) / np.float32(20.0)
        want = A.demap_f32(syms, n0, apsk_points(constellation, rate))[0]
        got = np.fromfile(fout, np.int8).reshape(3, -1)
        assert np.array_equal(got, want)
        n_llr = rows * A.N_MOD[constellation]
        assert f"frames 3 symbols_per_frame {rows} consumed {3 * rows} produced {3 * n_llr} found 3" in r.stdout, r.stdout
        refined = float(r.stdout.split("refined_snr_db")[1].split()[0])
        assert abs(refined - 10 * np.log10(np.mean(A.snr_f64(syms, p, want)))) < 1e-3
        assert "8APSK: Unsupported constellation" in r.stdout
