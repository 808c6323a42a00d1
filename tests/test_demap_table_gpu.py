"""GPU: the demapper of a caller's constellation table (dvbs2_demap_create_table, 4 .. 256 points, the caller's column order) -- bit
for bit against the float32 model of tests/apsk_model.py taken through column[] and under its float64 rule, the built-in 16APSK /
32APSK tables given as caller tables against the built-in handles, the SNR estimates against float64, end to end through
FecChain.from_table, the handle entries and the C++ host mirror. The tables are test material (tests/demap_table_model.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import apsk_model as A
import demap_table_model as D
import fec_testlib as T
from dvbs2rx_amd import Demapper, FecChain, apsk_points, capi

pytestmark = pytest.mark.gpu

PAD = 256


def _device_demap(dm, d_syms, n_frames, n0_ptr, n0_count):
    """(n_frames, n_llr) int8 from the device entry, with 0x5A canaries PAD bytes in front of and behind the output"""
    import torch
    d_out = torch.full((PAD + n_frames * dm.n_llr + PAD,), 0x5A, dtype=torch.int8, device="cuda")
    dm.work_device(d_syms.data_ptr(), n_frames, n0_ptr, n0_count, d_out.data_ptr() + PAD)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:PAD] == 0x5A).all() and (out[-PAD:] == 0x5A).all()
    return out[PAD:-PAD].reshape(n_frames, -1)


@pytest.mark.parametrize("name,table,framesize,column", D.CASES, ids=[c[0] for c in D.CASES])
def test_demap_bit_for_bit(name, table, framesize, column):
    import torch
    syms, nat_pf, nat_one, p, p32, one_n0 = D.demap_case(table, framesize)
    n_mod = int(np.log2(len(p)))
    rows = syms.shape[1]
    col = D.natural(n_mod) if column is None else list(column)
    want_pf, want_one = D.permute_columns(nat_pf, n_mod, col), D.permute_columns(nat_one, n_mod, col)
    dm = Demapper.from_table(framesize, p32, column, max_frames=3)
    assert (dm.n_syms, dm.n_mod, dm.n_llr, dm.column_order) == (rows, n_mod, rows * n_mod, 0 if col == D.natural(n_mod) else -1)
    keep, sel = D.unplanted(rows, n_mod)
    # host entry
    assert np.array_equal(dm.work(syms, D.N0_FRAMES), want_pf)
    assert np.array_equal(dm.work(syms, one_n0), want_one)
    # device entry, canaries around the output
    d_syms = torch.from_numpy(syms.view(np.float32).copy()).cuda()
    d_n0 = torch.from_numpy(np.concatenate([D.N0_FRAMES, [one_n0]]).astype(np.float32)).cuda()
    for n0_ptr, n0_count, n0, want in ((d_n0.data_ptr(), 3, D.N0_FRAMES, want_pf), (d_n0.data_ptr() + 12, 1, one_n0, want_one)):
        got = _device_demap(dm, d_syms, 3, n0_ptr, n0_count)
        A.check_vs_f64(D.unpermute_columns(got, n_mod, col)[:, sel], syms[:, keep], n0, p, name + " device")
        assert np.array_equal(got, want)
        if name == D.SATURATION_CASE and n0_count == 1:
            sat = np.mean((got[0] == 127) | (got[0] == -128))
            print(f"{name}: saturated share of frame 0 at N0 {one_n0} {sat:.3f}")
            assert 0.05 < sat < 0.25  # the run covers saturation
    # two frames of three: the third frame's bytes stay
    d_out = torch.full((3 * dm.n_llr,), 0x5A, dtype=torch.int8, device="cuda")
    dm.work_device(d_syms.data_ptr(), 2, d_n0.data_ptr(), 2, d_out.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().reshape(3, -1)
    assert np.array_equal(out[:2], want_pf[:2]) and (out[2] == 0x5A).all()
    dm.close()


@pytest.mark.parametrize("constellation,rate,rows", [(capi.MOD_16APSK, "C2_3", 4050), (capi.MOD_32APSK, "C3_4", 3240)], ids=["16apsk-2_3", "32apsk-3_4"])
def test_builtin_tables_as_caller_tables(constellation, rate, rows):
    """The new path against the merged one, independently of the model: the library's own 16APSK / 32APSK tables, given as caller
    tables, yield the bytes of the built-in handles; with the reversed column order, the same bytes with the columns reversed."""
    n_mod = A.N_MOD[constellation]
    rng = np.random.default_rng(rows)
    pts = apsk_points(constellation, rate)
    n0 = np.array([0.2, 0.05, 0.01], np.float32)
    tx = pts[rng.integers(0, len(pts), (3, rows))]
    syms = (tx + np.sqrt(n0.astype(np.float64) / 2.0)[:, None] * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))).astype(np.complex64)
    syms[:, [0, rows - 1]] = 0
    syms[:, [1, rows - 2]] = 1e3 - 1e3j
    built_in = Demapper(framesize=capi.FECFRAME_SHORT, rate=rate, constellation=constellation, max_frames=3)
    want = built_in.work(syms, n0)
    assert built_in.n_syms == rows
    for column in (None, D.natural(n_mod), list(range(n_mod - 1, -1, -1))):
        dm = Demapper.from_table(capi.FECFRAME_SHORT, pts, column, max_frames=3)
        got = dm.work(syms, n0)
        if column is not None and column[0] != 0:
            assert dm.column_order == -1
            got = np.ascontiguousarray(got.reshape(3, n_mod, rows)[:, ::-1, :]).reshape(3, -1)
        else:
            assert dm.column_order == 0
        assert np.array_equal(got, want)
        dm.close()
    built_in.close()


@pytest.mark.parametrize("name,table,framesize,column", [D.CASES[2], D.CASES[0]], ids=[D.CASES[2][0], D.CASES[0][0]])
def test_snr_estimates(name, table, framesize, column):
    import torch
    p = D.TABLES[table]
    n_mod = int(np.log2(len(p)))
    rows = D.N_LLR[framesize] // n_mod
    col = D.natural(n_mod) if column is None else list(column)
    sigma = np.array([0.01, 0.03, 0.06])
    rng = np.random.default_rng(rows)
    bits = rng.integers(0, 2, (3, rows * n_mod), dtype=np.uint8)
    tx = D.map_bits_columns(bits, p, col)
    syms = (tx + sigma[:, None] * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))).astype(np.complex64)
    llr = np.where(bits == 1, rng.integers(-128, 0, bits.shape), rng.integers(0, 128, bits.shape)).astype(np.int8)  # 0 counts as bit 0
    dm = Demapper.from_table(framesize, p, column, max_frames=3)
    pre, want_pre = dm.estimate_snr(syms), A.snr_f64(syms, p)
    post, want_post = dm.refine_snr(syms, llr), A.snr_f64(syms, p, D.unpermute_columns(llr, n_mod, col))  # the label through column[]
    print(f"{name}: estimate_snr {pre} (model {want_pre}), refine_snr {post} (model {want_post}), 1 / (2 sigma^2) {1 / (2 * sigma ** 2)}")
    assert np.allclose(pre, want_pre, rtol=2e-4, atol=0)
    assert np.allclose(post, want_post, rtol=2e-4, atol=0)
    sent = (np.abs(tx) ** 2).sum(axis=1) / (np.abs(syms.astype(np.complex128) - tx) ** 2).sum(axis=1)
    assert np.allclose(post, sent, rtol=2e-4, atol=0)  # the re-mapped points are the sent ones
    d_syms = torch.from_numpy(syms.view(np.float32).copy()).cuda()
    d_llr = torch.from_numpy(llr).cuda()
    d_snr = torch.zeros(6, dtype=torch.float32, device="cuda")
    capi.check(capi.lib.dvbs2_demap_estimate_snr_device(dm._h, d_syms.data_ptr(), 3, d_snr.data_ptr(), None))
    capi.check(capi.lib.dvbs2_demap_refine_snr_device(dm._h, d_syms.data_ptr(), d_llr.data_ptr(), 3, d_snr.data_ptr() + 12, None))
    torch.cuda.synchronize()
    assert np.array_equal(d_snr.cpu().numpy(), np.concatenate([pre, post]))
    dm.close()


@pytest.mark.parametrize("name", list(D.E2E))
def test_end_to_end_chain(name):
    """The operating points of test_demap_table_model.test_end_to_end_operating_point (Gray 64-QAM at 17.5 dB, Gray 256-QAM at
    22.5 dB, permuted columns, 8 short 3/4 frames, group of 8, 50 trials) through FecChain.from_table: the device entry and the
    host-buffer entry return every sent message, and the chain equals demapper -> chain from LLRs byte for byte."""
    import torch
    n_mod, column, es_n0_db = D.E2E[name]
    sent, cw, syms, n0, p = D.e2e_case(name)
    nf = D.E2E_FRAMES
    chain = FecChain.from_table(framesize=capi.FECFRAME_SHORT, rate="C3_4", points=p, column=column, group_size=D.E2E_GROUP, max_frames=nf,
                                max_trials=D.E2E_TRIALS)
    assert chain.n_syms == syms.shape[1] == 16200 // n_mod
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
    # enqueue + finish: the same bytes
    d_msg_q = torch.zeros_like(d_msg)
    chain.enqueue_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg_q.data_ptr())
    chain.finish()
    torch.cuda.synchronize()
    assert np.array_equal(d_msg_q.cpu().numpy(), sent)
    msg_host, ret_host, corr_host = chain.work(syms, n0)  # dvbs2_chain_decode: the chunked host pipeline
    assert np.array_equal(msg_host, sent) and (ret_host >= 0).all() and (corr_host >= 0).all()
    assert chain.fallback_rounds == 0
    # demapper -> chain from LLRs: the same bytes, return values and corrections
    dm = Demapper.from_table(capi.FECFRAME_SHORT, p, column, max_frames=nf)
    d_llr = torch.zeros((nf, dm.n_llr), dtype=torch.int8, device="cuda")
    dm.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_llr.data_ptr())
    torch.cuda.synchronize()
    llr = d_llr.cpu().numpy()
    assert np.array_equal(llr, D.permute_columns(A.demap_f32(syms, n0, p.astype(np.complex64))[0], n_mod, column))
    ber = np.mean((llr < 0).astype(np.uint8) != cw)
    print(f"{name} at {es_n0_db} dB: hard-decision bit error rate before the decoder {ber:.4f}, LDPC ret {ret_dev}, BCH corrections {corr_dev.sum()}")
    assert 1e-3 < ber < 0.1
    ll = FecChain(framesize=capi.FECFRAME_SHORT, rate="C3_4", group_size=D.E2E_GROUP, max_frames=nf, max_trials=D.E2E_TRIALS, from_llr=True)
    d_msg2, d_ret2, d_corr2 = torch.zeros_like(d_msg), torch.zeros_like(d_ret), torch.zeros_like(d_corr)
    ll.work_llr_device(d_llr.data_ptr(), nf, d_msg2.data_ptr(), d_ret2.data_ptr(), d_corr2.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_msg2.cpu().numpy(), msg_dev)
    assert np.array_equal(d_ret2.cpu().numpy(), ret_dev) and np.array_equal(d_corr2.cpu().numpy(), corr_dev)
    # the LLR forms of a table chain
    msg_llr, _, _ = chain.work_llr(llr)
    assert np.array_equal(msg_llr, sent)
    d_msg3 = torch.zeros_like(d_msg)
    chain.work_llr_device(d_llr.data_ptr(), nf, d_msg3.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_msg3.cpu().numpy(), sent)
    for o in (chain, dm, ll):
        o.close()


def test_handles():
    import torch
    lib = capi.lib
    name, table, framesize, column = D.CASES[2]
    syms, nat_pf, _, p, p32, _ = D.demap_case(table, framesize)
    n_mod, rows = 6, syms.shape[1]
    want = D.permute_columns(nat_pf, n_mod, column)
    dm = Demapper.from_table(framesize, p32, column, max_frames=1)
    for f in range(3):
        assert np.array_equal(dm.work(syms[f:f + 1], D.N0_FRAMES[f]), want[f:f + 1])
    # read back exactly what was given
    pts, col = dm.table()
    assert pts.tobytes() == p32.tobytes() and col.tolist() == list(column) and dm.column_order == -1
    n = C.c_int()
    assert lib.dvbs2_demap_table(dm._h, n, None, None) == capi.OK and n.value == n_mod
    nat = Demapper.from_table(framesize, p32, None, max_frames=1)
    assert nat.table()[1].tolist() == D.natural(n_mod) and nat.column_order == 0
    nat.close()
    built_in = Demapper(framesize=capi.FECFRAME_SHORT, rate="C2_3", constellation=capi.MOD_16APSK, max_frames=1)
    assert lib.dvbs2_demap_table(built_in._h, n, None, None) == capi.EINVAL and b"table" in lib.dvbs2_last_error()
    built_in.close()
    # zero-frame calls on every entry
    assert lib.dvbs2_demap_soft_device(dm._h, None, 0, None, 1, None, None) == capi.OK
    assert lib.dvbs2_demap_soft(dm._h, None, 0, None, 1, None) == capi.OK
    assert lib.dvbs2_demap_estimate_snr(dm._h, None, 0, None) == capi.OK
    assert lib.dvbs2_demap_estimate_snr_device(dm._h, None, 0, None, None) == capi.OK
    assert lib.dvbs2_demap_refine_snr(dm._h, None, None, 0, None) == capi.OK
    assert lib.dvbs2_demap_refine_snr_device(dm._h, None, None, 0, None, None) == capi.OK
    # more frames than the handle holds
    out = np.empty((2, dm.n_llr), np.int8)
    snr = np.empty(2, np.float32)
    two = np.ascontiguousarray(syms[:2])
    assert lib.dvbs2_demap_soft(dm._h, two.ctypes.data, 2, D.N0_FRAMES.ctypes.data, 1, out.ctypes.data) == capi.ESIZE
    assert lib.dvbs2_demap_estimate_snr(dm._h, two.ctypes.data, 2, snr.ctypes.data) == capi.ESIZE
    assert lib.dvbs2_demap_refine_snr(dm._h, two.ctypes.data, out.ctypes.data, 2, snr.ctypes.data) == capi.ESIZE
    dm.close()
    chain = FecChain.from_table(framesize=framesize, rate="C3_4", points=p32, column=column, group_size=4, max_frames=1, max_trials=5)
    assert chain.n_syms == rows and chain.n_llr == 16200
    d_msg = torch.zeros(chain.msg_bytes, dtype=torch.uint8, device="cuda")
    chain.work_device(0, 0, 0, 1, d_msg.data_ptr())
    chain.enqueue_device(0, 0, 0, 1, d_msg.data_ptr())
    chain.finish()
    chain.work_llr_device(0, 0, d_msg.data_ptr())
    msg, _, _ = chain.work(np.zeros((0, rows), np.complex64), 0.1)
    assert msg.shape == (0, chain.msg_bytes)
    assert chain.work_llr(np.zeros((0, 16200), np.int8))[0].shape == (0, chain.msg_bytes)
    msg2 = np.empty((2, chain.msg_bytes), np.uint8)
    assert lib.dvbs2_chain_decode(chain._h, two.ctypes.data, 2, D.N0_FRAMES.ctypes.data, 1, 5, msg2.ctypes.data, None, None) == capi.ESIZE
    chain.close()
    # refused arguments through create: the texts of the check, the handle stays null
    pf = np.ascontiguousarray(p32)
    nan = pf.copy()
    nan.view(np.float32)[9] = np.nan
    dup = np.array([0, 1, 2, 3, 4, 4], np.uint8)
    for n_mod_arg, pts_ptr, col_ptr, text in ((7, pf.ctypes.data, None, b"multiple of 7"), (9, pf.ctypes.data, None, b"n_mod"), (1, pf.ctypes.data, None, b"n_mod"),
                                              (6, None, None, b"points_re_im"), (6, nan.ctypes.data, None, b"points_re_im"), (6, pf.ctypes.data, dup.ctypes.data, b"column")):
        h = C.c_void_p(1)
        assert lib.dvbs2_demap_create_table(C.byref(h), framesize, n_mod_arg, pts_ptr, col_ptr, 4, 0) == capi.EINVAL and not h.value
        assert text in lib.dvbs2_last_error(), (n_mod_arg, lib.dvbs2_last_error())
        assert lib.dvbs2_demap_table_check(n_mod_arg, pts_ptr, col_ptr) == capi.EINVAL and text in lib.dvbs2_last_error()
        h = C.c_void_p(1)
        assert lib.dvbs2_chain_create_table(C.byref(h), capi.STANDARD_DVBS2, framesize, 6, n_mod_arg, pts_ptr, col_ptr, 4, 4, 0) == capi.EINVAL and not h.value
        assert text in lib.dvbs2_last_error()
    h = C.c_void_p(1)
    assert lib.dvbs2_demap_create_table(C.byref(h), 5, 6, pf.ctypes.data, None, 4, 0) == capi.EINVAL and not h.value and b"framesize" in lib.dvbs2_last_error()
    h = C.c_void_p(1)
    assert lib.dvbs2_demap_create_table(C.byref(h), framesize, 6, pf.ctypes.data, None, 0, 0) == capi.EINVAL and not h.value and b"max_frames" in lib.dvbs2_last_error()


def test_host_mirror(tmp_path):
    """xfecframe_demapper_cb::make_table of host/dvbs2rx_hip_blocks.h on the 64-point ring table with permuted columns: the model's
    bytes, and the llr_pdu refinement within 1e-3 dB of the float64 model."""
    libdir = os.path.join(T.ROOT, "gr-dvbs2rx_amd", "lib")
    exe = str(tmp_path / "demap_table_host_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(T.ROOT, "tests", "demap_table_host_main.cpp"), "-o", exe,
                           "-L" + libdir, "-ldvbs2_fec_hip", "-Wl,-rpath," + libdir])
    name, table, framesize, column = D.CASES[2]
    syms, _, _, p, p32, _ = D.demap_case(table, framesize)
    n_mod, rows = 6, syms.shape[1]
    fin, fout, ftab = str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "table.bin")
    syms.tofile(fin)
    p32.tofile(ftab)
    r = subprocess.run([exe, fin, fout, ftab, str(framesize), str(n_mod), "".join(str(c) for c in column), "200.0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    n0 = np.float32(1.0) / np.float32(200.0)
    nat = A.demap_f32(syms, n0, p32)[0]
    got = np.fromfile(fout, np.int8).reshape(3, -1)
    assert np.array_equal(got, D.permute_columns(nat, n_mod, column))
    assert f"frames 3 symbols_per_frame {rows} consumed {3 * rows} produced {3 * rows * n_mod} found 3" in r.stdout, r.stdout
    refined = float(r.stdout.split("refined_snr_db")[1].split()[0])
    assert abs(refined - 10 * np.log10(np.mean(A.snr_f64(syms, p, nat)))) < 1e-3
    assert "n_mod 7: " in r.stdout and "multiple of 7" in r.stdout
