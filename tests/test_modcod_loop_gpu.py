"""Every DVB-S2 MODCOD round the transmit-receive loop on the device, noise-free: FecEncoder -> PlFramer -> a constant phase ->
PlFrontEnd -> FecChain returns the sent bytes, and the four handles agree on every size. Then one VCM stream with four MODCODs and
dummy frames through PlSync, gather per PLSC, and a front end and a chain per MODCOD. Geometry, labels and column order agreeing
between the two halves is the point; the noisy comparison with the CPU chain is test_demap_paths_gpu.py."""
import numpy as np
import pytest

import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import FecChain, FecEncoder, PlFramer, PlFrontEnd, PlSync, capi, enc_check, get_fec_info, plframer_layout
from fec_testlib import stream

SHORT, NORMAL = capi.FECFRAME_SHORT, capi.FECFRAME_NORMAL
# EN 302 307-1 table 12: MODCOD -> (rate, constellation)
MODCODS = {1: ("C1_4", capi.MOD_QPSK), 2: ("C1_3", capi.MOD_QPSK), 3: ("C2_5", capi.MOD_QPSK), 4: ("C1_2", capi.MOD_QPSK),
           5: ("C3_5", capi.MOD_QPSK), 6: ("C2_3", capi.MOD_QPSK), 7: ("C3_4", capi.MOD_QPSK), 8: ("C4_5", capi.MOD_QPSK),
           9: ("C5_6", capi.MOD_QPSK), 10: ("C8_9", capi.MOD_QPSK), 11: ("C9_10", capi.MOD_QPSK),
           12: ("C3_5", capi.MOD_8PSK), 13: ("C2_3", capi.MOD_8PSK), 14: ("C3_4", capi.MOD_8PSK), 15: ("C5_6", capi.MOD_8PSK),
           16: ("C8_9", capi.MOD_8PSK), 17: ("C9_10", capi.MOD_8PSK),
           18: ("C2_3", capi.MOD_16APSK), 19: ("C3_4", capi.MOD_16APSK), 20: ("C4_5", capi.MOD_16APSK), 21: ("C5_6", capi.MOD_16APSK),
           22: ("C8_9", capi.MOD_16APSK), 23: ("C9_10", capi.MOD_16APSK),
           24: ("C3_4", capi.MOD_32APSK), 25: ("C4_5", capi.MOD_32APSK), 26: ("C5_6", capi.MOD_32APSK), 27: ("C8_9", capi.MOD_32APSK),
           28: ("C9_10", capi.MOD_32APSK)}
N_MOD = {capi.MOD_QPSK: 2, capi.MOD_8PSK: 3, capi.MOD_16APSK: 4, capi.MOD_32APSK: 5}
LEGAL = [(m, fs) for m in MODCODS for fs in (NORMAL, SHORT) if not (fs == SHORT and MODCODS[m][0] == "C9_10")]  # 9/10 has no short frame
GOLD = 5


def plsc_of(modcod, framesize, pilots):
    return P.plsc_of(modcod, int(framesize == SHORT), int(pilots))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ the table, without a device
def test_modcod_table_sizes_and_legal_combinations():
    """For all 28 MODCODs and both frame sizes the FEC parameters and the PL signalling give the same XFECFRAME length, and the
    encoder takes exactly the 52 combinations of the standard."""
    assert sorted(MODCODS) == list(range(1, 29)) and len(LEGAL) == 52
    taken = []
    for modcod, (rate, constellation) in MODCODS.items():
        for fs in (NORMAL, SHORT):
            try:
                enc_check(capi.STANDARD_DVBS2, fs, rate, constellation)
            except capi.Dvbs2Error as e:
                assert e.code == capi.EINVAL, (modcod, fs)
                continue
            taken.append((modcod, fs))
            info = M.pls_parse(plsc_of(modcod, fs, 1))
            assert info["n_mod"] == N_MOD[constellation], modcod
            assert get_fec_info(capi.STANDARD_DVBS2, fs, rate)["ldpc_n"] // N_MOD[constellation] == info["xfecframe_len"], (modcod, fs)
    assert taken == LEGAL


# ------------------------------------------------------------------ one MODCOD at a time
PILOTLESS = [(4, SHORT), (13, SHORT), (18, SHORT), (24, SHORT)]  # one of each constellation
LOOP = [(m, fs, 1) for m, fs in LEGAL] + [(m, fs, 0) for m, fs in PILOTLESS]


@pytest.mark.gpu
@pytest.mark.parametrize("modcod,fs,pilots", LOOP, ids=["modcod%d-%s-%s" % (m, "short" if fs == SHORT else "normal", "pilots" if p else "nopilots")
                                                        for m, fs, p in LOOP])
def test_every_modcod_round_the_loop(modcod, fs, pilots):
    import torch
    rate, constellation = MODCODS[modcod]
    plsc, nf = plsc_of(modcod, fs, pilots), 3
    info = M.pls_parse(plsc)
    enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, constellation, max_frames=nf)
    enc.set_scramble(True)
    fr = PlFramer(GOLD, max_frames=nf)
    fr.set_sequence([plsc] * nf)
    fe = PlFrontEnd(GOLD, plsc, max_frames=nf)
    chain = FecChain(capi.STANDARD_DVBS2, fs, rate, constellation, group_size=4, max_frames=nf)
    chain.set_descramble(True)
    # the four handles and the PL signalling agree on every size
    assert enc.n_syms == fe.xfecframe_len == chain.n_syms == info["xfecframe_len"]
    assert enc.n_mod == fe.n_mod == N_MOD[constellation] and enc.ldpc_n == chain.n_llr == enc.n_syms * enc.n_mod
    assert enc.in_bytes == chain.msg_bytes == get_fec_info(capi.STANDARD_DVBS2, fs, rate)["bch_k"] // 8
    assert (fr.n_frames, fr.in_syms, fr.out_syms) == (nf, nf * enc.n_syms, nf * fe.plframe_len)
    assert (fe.plframe_len, fe.n_slots, fe.n_pilots) == (info["plframe_len"], info["n_slots"], info["n_pilots"])
    assert (fe.n_pilots > 0) == bool(pilots)
    sent = np.random.default_rng(100 * modcod + 2 * fs + pilots).integers(0, 256, (nf, enc.in_bytes), dtype=np.uint8)
    d_xfec = torch.zeros((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda")
    enc.work_device(dev(sent).data_ptr(), nf, d_syms=d_xfec.data_ptr(), stream=stream())
    d_pl = torch.zeros((fr.out_syms + 90, 2), dtype=torch.float32, device="cuda")
    fr.work_device(d_xfec.data_ptr(), nf, plsc, d_pl.data_ptr(), stream())
    phasor = complex(np.exp(2.1j))
    d_rot = torch.view_as_real(torch.view_as_complex(d_pl) * phasor).contiguous()
    cc = torch.ones(nf, dtype=torch.int32, device="cuda")
    cf = torch.zeros(nf, dtype=torch.float32, device="cuda")
    d_rx = torch.zeros((nf, fe.xfecframe_len, 2), dtype=torch.float32, device="cuda")
    d_p = torch.zeros(nf, dtype=torch.uint8, device="cuda")
    fe.work_device(d_rot.data_ptr(), nf, 1, cc.data_ptr(), 0 if pilots else cf.data_ptr(), d_rx.data_ptr(), stream(), plsc_decoded=d_p.data_ptr())
    d_n0 = torch.full((1,), 0.02, dtype=torch.float32, device="cuda")
    d_msg = torch.zeros((nf, chain.msg_bytes), dtype=torch.uint8, device="cuda")
    d_ret = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_corr = torch.full((nf,), -7, dtype=torch.int32, device="cuda")
    chain.work_device(d_rx.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr(), stream())
    torch.cuda.synchronize()
    fallback = chain.fallback_rounds
    for o in (chain, fe, fr, enc):
        o.close()
    assert d_p.cpu().tolist() == [plsc] * nf
    assert (d_ret.cpu().numpy() >= 0).all(), d_ret.cpu().tolist()
    assert (d_corr.cpu().numpy() == 0).all(), d_corr.cpu().tolist()
    assert np.array_equal(d_msg.cpu().numpy(), sent)
    assert fallback == 0


# ------------------------------------------------------------------ one stream, four MODCODs
@pytest.mark.gpu
def test_vcm_stream_round_the_loop():
    """Short frames of QPSK 1/2 (pilots), 8PSK 3/5 (no pilots), 16APSK 3/4 (pilots), 32APSK 4/5 (pilots) and two dummy frames in one
    stream behind an odd lead: PlSync(plsc=-1) finds every frame where the framer's layout puts it; for each data PLSC the gathered
    frames are its locked records, and their bytes are the encoder inputs of exactly those frames."""
    import torch
    a, b, c, d, dummy = plsc_of(4, SHORT, 1), plsc_of(12, SHORT, 0), plsc_of(19, SHORT, 1), plsc_of(25, SHORT, 1), P.plsc_of(0, 0, 0)
    seq = [a, a, b, c, d, dummy, b, a, d, c, dummy, c, d, b, a, b, c, d]
    data_plscs = (a, b, c, d)
    assert all(seq.count(p) >= 4 for p in data_plscs) and seq.count(dummy) == 2
    rng = np.random.default_rng(2026)
    lay = plframer_layout(seq)
    d_xfec = torch.zeros((lay["in_syms"], 2), dtype=torch.float32, device="cuda")
    sent = {}
    for p in data_plscs:
        rate, constellation = MODCODS[p >> 2]
        where = [f for f, q in enumerate(seq) if q == p]
        enc = FecEncoder(capi.STANDARD_DVBS2, SHORT, rate, constellation, max_frames=len(where))
        enc.set_scramble(True)
        assert enc.n_syms == M.pls_parse(p)["xfecframe_len"]
        sent[p] = rng.integers(0, 256, (len(where), enc.in_bytes), dtype=np.uint8)
        d_one = torch.zeros((len(where), enc.n_syms, 2), dtype=torch.float32, device="cuda")
        enc.work_device(dev(sent[p]).data_ptr(), len(where), d_syms=d_one.data_ptr(), stream=stream())
        for k, f in enumerate(where):  # the framer reads the XFECFRAMEs of the data frames back to back in stream order
            i = int(lay["in_offset"][f])
            d_xfec[i:i + enc.n_syms] = d_one[k]
        torch.cuda.synchronize()
        enc.close()
    assert lay["in_syms"] == sum(M.pls_parse(q)["xfecframe_len"] for q in seq if q != dummy)
    fr = PlFramer(GOLD, max_frames=len(seq))
    fr.set_sequence(seq)
    lead, tail = 301, 300  # an odd lead: the frames start 8-byte aligned in the stream
    n = lead + lay["out_syms"] + 90 + tail
    noise = np.concatenate([P.qpsk(rng, lead), P.qpsk(rng, tail)]).astype(np.complex64)
    d_x = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    d_x[:lead] = dev(noise[:lead].view(np.float32).reshape(-1, 2))
    d_x[n - tail:] = dev(noise[lead:].view(np.float32).reshape(-1, 2))
    fr.work_device(d_xfec.data_ptr(), len(seq), seq[-1], d_x.data_ptr() + 8 * lead, stream())
    # search
    ps = PlSync(plsc=-1, max_symbols=max(n, PlSync.MIN_SYMBOLS), max_frames=64)
    d_f = torch.zeros(ps.max_frames * 16, dtype=torch.uint8, device="cuda")
    ps.work_device(d_x.data_ptr(), n, d_f.data_ptr(), stream())
    nrec, consumed, state = ps.finish()
    recs = d_f.cpu().numpy().view(PlSync.FRAME_DTYPE)[:nrec]
    assert recs["sof_index"].tolist() == (lead + lay["out_offset"]).tolist()
    assert recs["plsc"].tolist() == seq and state == capi.PLSYNC_LOCKED
    # per PLSC: gather, front end, chain
    for p in data_plscs:
        rate, constellation = MODCODS[p >> 2]
        info = M.pls_parse(p)
        locked = [f for f, r in enumerate(recs) if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == p]
        assert len(locked) >= 3, p
        d_fr = torch.zeros((len(locked) * info["plframe_len"] + 90) * 2, dtype=torch.float32, device="cuda")
        d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        ps.gather_device(d_x.data_ptr(), d_f.data_ptr(), nrec, p, d_fr.data_ptr(), d_cnt.data_ptr(), stream())
        torch.cuda.synchronize()
        cnt = int(d_cnt.item())
        assert cnt == len(locked), p  # all locked frames of this PLSC are gathered, and no other
        fe = PlFrontEnd(GOLD, p, max_frames=cnt)
        assert fe.plframe_len == info["plframe_len"]
        cc = torch.ones(cnt, dtype=torch.int32, device="cuda")
        cf = torch.zeros(cnt, dtype=torch.float32, device="cuda")
        d_rx = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
        d_p = torch.zeros(cnt, dtype=torch.uint8, device="cuda")
        fe.work_device(d_fr.data_ptr(), cnt, 1, cc.data_ptr(), 0 if info["has_pilots"] else cf.data_ptr(), d_rx.data_ptr(), stream(),
                       plsc_decoded=d_p.data_ptr())
        chain = FecChain(capi.STANDARD_DVBS2, SHORT, rate, constellation, group_size=4, max_frames=cnt)
        chain.set_descramble(True)
        assert chain.n_syms == fe.xfecframe_len
        d_n0 = torch.full((1,), 0.02, dtype=torch.float32, device="cuda")
        d_msg = torch.zeros((cnt, chain.msg_bytes), dtype=torch.uint8, device="cuda")
        d_ret = torch.full(((cnt + 3) // 4,), -7, dtype=torch.int32, device="cuda")
        d_corr = torch.full((cnt,), -7, dtype=torch.int32, device="cuda")
        chain.work_device(d_rx.data_ptr(), cnt, d_n0.data_ptr(), 1, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr(), stream())
        torch.cuda.synchronize()
        chain.close()
        fe.close()
        assert d_p.cpu().tolist() == [p] * cnt
        assert (d_ret.cpu().numpy() >= 0).all() and (d_corr.cpu().numpy() >= 0).all(), p
        data_index = [sum(1 for q in seq[:f] if q == p) for f in locked]  # which encoder frame each gathered frame carries
        assert np.array_equal(d_msg.cpu().numpy(), sent[p][data_index]), p
    ps.close()
    fr.close()
