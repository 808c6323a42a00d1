"""PL framer on the device (dvbs2_plframer_*) against the float32 model of tests/plframer_model.py: every output BIT FOR BIT (uint32
compare) -- the framer is a swap, a sign flip and copies of constants --, then the receive stages in a closed loop on what it wrote."""
import ctypes as C

import numpy as np
import pytest

import plframe_model as M
import plframer_model as F
import plsync_model as P
from dvbs2rx_amd import FecChain, FecEncoder, PlFramer, PlFrontEnd, PlSync, capi, plframer_layout
from fec_testlib import SENTINEL, refused, sentinel, stream

pytestmark = pytest.mark.gpu

PAD = 64               # sentinel symbols beyond the end


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frame_on_device(fr, data, n_frames, closing, n_out, in_shift=0, out_shift=0):
    """One frame_device call into a sentinel buffer of n_out + PAD symbols. The shifts displace the buffers by that many symbols (8 bytes
    each) from torch's allocation. Returns every symbol of the buffer from the (displaced) start, as uint32 (n, 2)."""
    import torch
    d_in = torch.zeros(((data.shape[0] + in_shift) * 2 + 4,), dtype=torch.float32, device="cuda")
    if data.size:
        d_in[2 * in_shift:2 * (in_shift + data.shape[0])] = dev(data.reshape(-1))
    d_out = sentinel(2 * (n_out + out_shift + PAD))
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    fr.work_device(d_in.data_ptr() + 8 * in_shift if data.size else 0, n_frames, closing, d_out.data_ptr() + 8 * out_shift, stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)[out_shift:]


def check_against_model(got, want):
    """got: the whole sentinel buffer; want: (n, 2) float32. The first n symbols are the model's bits, everything behind is untouched."""
    n = want.shape[0]
    assert got.shape[0] == n + PAD
    assert np.array_equal(got[:n], F.bits(want))
    assert (got[n:] == SENTINEL).all()


# ------------------------------------------------------------------ 1. bits against the model, one geometry each
GEOMETRIES = [P.plsc_of(0, 0, 0), P.plsc_of(0, 0, 1), P.plsc_of(4, 1, 0), P.plsc_of(4, 1, 1), P.plsc_of(13, 1, 1), P.plsc_of(18, 1, 1),
              P.plsc_of(24, 1, 1), P.plsc_of(24, 0, 1)]
EXPECTED_GEOMETRY = {P.plsc_of(0, 0, 0): (36, 0), P.plsc_of(0, 0, 1): (36, 0), P.plsc_of(4, 1, 0): (90, 0), P.plsc_of(4, 1, 1): (90, 5),
                     P.plsc_of(13, 1, 1): (60, 3), P.plsc_of(18, 1, 1): (45, 2), P.plsc_of(24, 1, 1): (36, 2), P.plsc_of(24, 0, 1): (144, 8),
                     P.plsc_of(4, 0, 1): (360, 22)}
CASES_1 = [(p, g, (1, 3)) for p in GEOMETRIES for g in (0, 5, 262142)] + [(P.plsc_of(4, 0, 1), 5, (1,))]


@pytest.mark.parametrize("plsc,gold,counts", CASES_1, ids=[f"plsc{p}-gold{g}" for p, g, _ in CASES_1])
def test_bits_equal_the_model(plsc, gold, counts):
    info = M.pls_parse(plsc)
    assert (info["n_slots"], info["n_pilots"]) == EXPECTED_GEOMETRY[plsc]
    fr = PlFramer(gold, max_frames=max(counts))
    for nf in counts:
        seq = [plsc] * nf
        lay = F.layout(seq)
        data = F.planted_data(np.random.default_rng(1000 * plsc + nf), lay["in_syms"]) if lay["in_syms"] else np.zeros((0, 2), np.float32)
        fr.set_sequence(seq)
        assert (fr.n_frames, fr.in_syms, fr.out_syms) == (nf, lay["in_syms"], lay["out_syms"])
        for closing in (-1, plsc ^ 1):  # the other header of the same geometry
            want = F.frames(seq, gold, data, closing)
            check_against_model(frame_on_device(fr, data, nf, closing, want.shape[0]), want)
    fr.close()


# ------------------------------------------------------------------ 2. a sequence with mixed MODCODs; 3. alignment; 6. host entry
@pytest.fixture(scope="module")
def acm():
    seq = list(P.ACM_PLSCS)
    lay = F.layout(seq)
    data = F.planted_data(np.random.default_rng(77), lay["in_syms"])
    return dict(seq=seq, lay=lay, data=data, gold=3, want=F.frames(seq, 3, data, seq[-1]))


def test_sequence_with_mixed_modcods(acm):
    seq, lay, data, gold = acm["seq"], acm["lay"], acm["data"], acm["gold"]
    assert len(seq) == 13 and sum(M.pls_parse(p)["dummy_frame"] for p in seq) == 2
    mine = plframer_layout(seq)
    assert mine["out_offset"].tolist() == lay["out_offset"].tolist() and mine["in_offset"].tolist() == lay["in_offset"].tolist()
    fr = PlFramer(gold, max_frames=13)
    fr.set_sequence(seq)
    got = frame_on_device(fr, data, 13, seq[-1], lay["out_syms"] + 90)
    check_against_model(got, acm["want"])
    for f, (p, o) in enumerate(zip(seq, mine["out_offset"])):  # frame by frame at the offsets of plframer_layout
        info = M.pls_parse(p)
        i = int(mine["in_offset"][f])
        one = F.frame(p, gold, None if info["dummy_frame"] else data[i:i + info["xfecframe_len"]])
        assert np.array_equal(got[o:o + info["plframe_len"]], F.bits(one)), f
    # without a closing header: 90 symbols fewer
    check_against_model(frame_on_device(fr, data, 13, -1, lay["out_syms"]), acm["want"][:-90])
    # the first 5 only: everything past out_offset[5] + 90 is still the sentinel
    end5 = int(mine["out_offset"][5])
    want5 = F.frames(seq[:5], gold, data[:int(mine["in_offset"][5])], seq[4])
    assert want5.shape[0] == end5 + 90
    got5 = frame_on_device(fr, data, 5, seq[4], lay["out_syms"] + 90)
    assert np.array_equal(got5[:end5 + 90], F.bits(want5)) and (got5[end5 + 90:] == SENTINEL).all()
    got5 = frame_on_device(fr, data, 5, -1, lay["out_syms"] + 90)
    assert np.array_equal(got5[:end5], F.bits(want5[:-90])) and (got5[end5:] == SENTINEL).all()
    fr.close()


@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_alignment(acm, in_shift, out_shift):
    """Buffers displaced by one symbol are 8-byte but not 16-byte aligned: the 8-byte path, the same bits."""
    fr = PlFramer(acm["gold"], max_frames=13)
    fr.set_sequence(acm["seq"])
    got = frame_on_device(fr, acm["data"], 13, acm["seq"][-1], acm["lay"]["out_syms"] + 90, in_shift, out_shift)
    check_against_model(got, acm["want"])
    fr.close()


def test_host_entry(acm):
    fr = PlFramer(acm["gold"], max_frames=13)
    fr.set_sequence(acm["seq"])
    x = acm["data"].view(np.complex64).reshape(-1)
    got = fr.work(x, closing_plsc=acm["seq"][-1])
    assert np.array_equal(got.view(np.uint32).reshape(-1, 2), F.bits(acm["want"]))
    got = fr.work(x[:int(acm["lay"]["in_offset"][5])], n_frames=5)
    assert np.array_equal(got.view(np.uint32).reshape(-1, 2), F.bits(acm["want"][:int(acm["lay"]["out_offset"][5])]))
    # dummy frames only: no input at all
    fr.set_sequence([0, 1])
    got = fr.work(np.zeros(0, np.complex64), closing_plsc=0)
    assert np.array_equal(got.view(np.uint32).reshape(-1, 2), F.bits(F.frames([0, 1], acm["gold"], np.zeros((0, 2), np.float32), 0)))
    fr.close()


# ------------------------------------------------------------------ 4. the inverse of the payload step
@pytest.mark.parametrize("plsc", [P.plsc_of(4, 1, 1), P.plsc_of(4, 1, 0), P.plsc_of(24, 0, 1)])
def test_inverse_of_the_payload_step(plsc):
    """Framer output through dvbs2_plpayload_process_device with zero phases returns the input with ==, not bits: the payload step's
    x * 1 - y * (-0) can change the sign of a zero."""
    import torch
    info, gold, nf = M.pls_parse(plsc), 11, 2
    assert info["n_slots"] in (90, 144)
    data = F.planted_data(np.random.default_rng(plsc), nf * info["xfecframe_len"])
    fr = PlFramer(gold, max_frames=nf)
    fr.set_sequence([plsc] * nf)
    d_in = dev(data.reshape(-1))
    d_out = torch.zeros((nf, info["plframe_len"], 2), dtype=torch.float32, device="cuda")
    fr.work_device(d_in.data_ptr(), nf, -1, d_out.data_ptr(), stream())
    d_pay = d_out[:, 90:].contiguous()
    h = C.c_void_p()
    capi.check(capi.lib.dvbs2_plpayload_create(C.byref(h), gold, info["n_slots"], info["has_pilots"], nf, 0))
    zf = torch.zeros((nf * max(info["n_pilots"], 1),), dtype=torch.float32, device="cuda")
    zi = torch.zeros((nf,), dtype=torch.int32, device="cuda")  # coarse_corrected = 0: the rotator runs on from the header phase, 0
    d_back = torch.full((nf * info["xfecframe_len"], 2), 9.0, dtype=torch.float32, device="cuda")
    capi.check(capi.lib.dvbs2_plpayload_process_device(h, d_pay.data_ptr(), nf, zf.data_ptr(), zf.data_ptr(), zi.data_ptr(), zf.data_ptr(),
                                                       d_back.data_ptr(), stream()))
    torch.cuda.synchronize()
    back = d_back.cpu().numpy()
    capi.lib.dvbs2_plpayload_destroy(h)
    fr.close()
    assert (back == data).all()


# ------------------------------------------------------------------ 5. closed loop through the receiver, noise-free
def test_closed_loop_through_the_receiver():
    import torch
    gold, plsc, dummy, nd = 5, P.plsc_of(1, 1, 1), P.plsc_of(0, 0, 0), 6
    rng = np.random.default_rng(2025)
    enc = FecEncoder(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, max_frames=nd)
    enc.set_scramble(True)
    sent = rng.integers(0, 256, (nd, enc.in_bytes), dtype=np.uint8)
    seq = [plsc, plsc, dummy, plsc, plsc, dummy, plsc, plsc]  # a dummy frame after data frames 2 and 4
    lay = plframer_layout(seq)
    L = M.pls_parse(plsc)["plframe_len"]
    assert enc.n_syms == M.pls_parse(plsc)["xfecframe_len"] and lay["in_syms"] == nd * enc.n_syms
    d_xfec = torch.zeros((nd, enc.n_syms, 2), dtype=torch.float32, device="cuda")
    enc.work_device(dev(sent).data_ptr(), nd, d_syms=d_xfec.data_ptr(), stream=stream())
    fr = PlFramer(gold, max_frames=len(seq))
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
    # gather the data frames, front end, chain
    locked = [f for f, r in enumerate(recs) if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == plsc]
    assert len(locked) >= nd - 1  # the tracker locks at the second header
    d_fr = torch.zeros((len(locked) * L + 90) * 2, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ps.gather_device(d_x.data_ptr(), d_f.data_ptr(), nrec, plsc, d_fr.data_ptr(), d_cnt.data_ptr(), stream())
    torch.cuda.synchronize()
    cnt = int(d_cnt.item())
    assert cnt == len(locked)  # all locked data frames are gathered
    fe = PlFrontEnd(gold, plsc, max_frames=cnt)
    cc = torch.ones(cnt, dtype=torch.int32, device="cuda")
    d_rx = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
    d_p = torch.zeros(cnt, dtype=torch.uint8, device="cuda")
    fe.work_device(d_fr.data_ptr(), cnt, 1, cc.data_ptr(), 0, d_rx.data_ptr(), stream(), plsc_decoded=d_p.data_ptr())
    torch.cuda.synchronize()
    assert d_p.cpu().tolist() == [plsc] * cnt
    chain = FecChain(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, group_size=4, max_frames=cnt, max_trials=25)
    chain.set_descramble(True)
    msg, ret, corr = chain.work(d_rx.cpu().numpy().view(np.complex64), np.float32(0.02))
    assert (ret >= 0).all() and (corr >= 0).all()
    data_index = [sum(1 for q in seq[:f] if q == plsc) for f in locked]  # which encoder frame each gathered frame carries
    assert np.array_equal(msg, sent[data_index])
    for o in (chain, fe, ps, fr, enc):
        o.close()


# ------------------------------------------------------------------ 7. arguments
def test_arguments(acm):
    import torch
    lib, h = capi.lib, C.c_void_p()
    # creation: the ranges of dvbs2_plpayload_create
    refused(capi.EINVAL, "gold code out of range", lib.dvbs2_plframer_create, C.byref(h), -1, 4, 0)
    refused(capi.EINVAL, "gold code out of range", lib.dvbs2_plframer_create, C.byref(h), (1 << 18) - 1, 4, 0)
    refused(capi.EINVAL, "max_frames must be in 1..65535 (frames are one launch dimension)", lib.dvbs2_plframer_create, C.byref(h), 0, 0, 0)
    refused(capi.EINVAL, "max_frames must be in 1..65535 (frames are one launch dimension)", lib.dvbs2_plframer_create, C.byref(h), 0, 65536, 0)
    assert not h
    refused(capi.EINVAL, "null handle pointer", lib.dvbs2_plframer_create, None, 0, 4, 0)

    seq, data, gold = acm["seq"][:5], acm["data"], acm["gold"]
    lay = F.layout(seq)
    want = F.frames(seq, gold, data[:lay["in_syms"]], seq[0])
    fr = PlFramer(gold, max_frames=6)
    d_in = dev(data[:lay["in_syms"]].reshape(-1))
    d_out = sentinel(2 * (lay["out_syms"] + 90 + PAD))
    st = stream()

    def good():
        """a good call follows every refusal and matches the model: the handle stays usable"""
        assert (fr.n_frames, fr.in_syms, fr.out_syms) == (5, lay["in_syms"], lay["out_syms"])
        d_out.fill_(np.uint32(SENTINEL).astype(np.int32).item())
        fr.work_device(d_in.data_ptr(), 5, seq[0], d_out.data_ptr(), st)
        torch.cuda.synchronize()
        check_against_model(d_out.cpu().numpy().view(np.uint32).reshape(-1, 2), want)

    def untouched():
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()

    # a fresh handle has an empty sequence
    assert (fr.n_frames, fr.in_syms, fr.out_syms) == (0, 0, 0)
    refused(capi.ESIZE, "n_frames exceeds the sequence", lib.dvbs2_plframer_frame_device, fr._h, d_in.data_ptr(), 1, -1, d_out.data_ptr(), st)
    assert lib.dvbs2_plframer_frame_device(fr._h, None, 0, -1, None, st) == capi.OK
    untouched()
    fr.set_sequence(seq)
    good()
    # set_sequence
    bad = np.array(seq, np.uint8)
    for value, why in ((128, "out of range (0..127)"), (29 << 2, "names a reserved MODCOD (29..31)"), ((31 << 2) | 3, "names a reserved MODCOD (29..31)")):
        bad[3] = value
        refused(capi.EINVAL, f"plsc[3] {why}", lib.dvbs2_plframer_set_sequence, fr._h, bad.ctypes.data, 5)
        good()
    seven = np.zeros(7, np.uint8)
    refused(capi.ESIZE, "n_frames exceeds max_frames", lib.dvbs2_plframer_set_sequence, fr._h, seven.ctypes.data, 7)
    good()
    refused(capi.EINVAL, "bad argument", lib.dvbs2_plframer_set_sequence, fr._h, None, 2)
    refused(capi.EINVAL, "bad argument", lib.dvbs2_plframer_set_sequence, fr._h, seven.ctypes.data, -1)
    good()
    # frame_device
    d_out.fill_(np.uint32(SENTINEL).astype(np.int32).item())
    a = (fr._h, d_in.data_ptr())
    refused(capi.ESIZE, "n_frames exceeds the sequence", lib.dvbs2_plframer_frame_device, *a, 6, -1, d_out.data_ptr(), st)
    refused(capi.EINVAL, "n_frames is negative", lib.dvbs2_plframer_frame_device, *a, -1, -1, d_out.data_ptr(), st)
    refused(capi.EINVAL, "closing_plsc out of range (-1 = none, 0..127)", lib.dvbs2_plframer_frame_device, *a, 5, 128, d_out.data_ptr(), st)
    refused(capi.EINVAL, "closing_plsc out of range (-1 = none, 0..127)", lib.dvbs2_plframer_frame_device, *a, 5, -2, d_out.data_ptr(), st)
    refused(capi.EINVAL, "closing_plsc names a reserved MODCOD (29..31)", lib.dvbs2_plframer_frame_device, *a, 5, 30 << 2, d_out.data_ptr(), st)
    refused(capi.EINVAL, "plframes is null", lib.dvbs2_plframer_frame_device, *a, 5, -1, None, st)
    refused(capi.EINVAL, "xfecframes is null and the framed prefix holds a data frame", lib.dvbs2_plframer_frame_device, fr._h, None, 5, -1,
            d_out.data_ptr(), st)
    refused(capi.EINVAL, "symbol buffers must be 8-byte aligned", lib.dvbs2_plframer_frame_device, fr._h, d_in.data_ptr() + 4, 5, -1,
            d_out.data_ptr(), st)
    assert lib.dvbs2_plframer_frame_device(*a, 0, -1, d_out.data_ptr(), st) == capi.OK  # n_frames == 0 writes nothing
    untouched()
    good()
    # the host entry makes the same checks
    host_in, host_out = data[:lay["in_syms"]].copy(), np.zeros((lay["out_syms"] + 90, 2), np.float32)
    refused(capi.ESIZE, "n_frames exceeds the sequence", lib.dvbs2_plframer_frame, fr._h, host_in.ctypes.data, 6, -1, host_out.ctypes.data)
    refused(capi.EINVAL, "closing_plsc names a reserved MODCOD (29..31)", lib.dvbs2_plframer_frame, fr._h, host_in.ctypes.data, 5, 29 << 2, host_out.ctypes.data)
    refused(capi.EINVAL, "plframes is null", lib.dvbs2_plframer_frame, fr._h, host_in.ctypes.data, 5, -1, None)
    refused(capi.EINVAL, "xfecframes is null and the framed prefix holds a data frame", lib.dvbs2_plframer_frame, fr._h, None, 5, -1, host_out.ctypes.data)
    assert lib.dvbs2_plframer_frame(fr._h, host_in.ctypes.data, 5, seq[0], host_out.ctypes.data) == capi.OK
    assert np.array_equal(F.bits(host_out), F.bits(want))
    good()
    # a prefix of dummy frames needs no input
    fr.set_sequence([1, 0] + seq[:3])
    want2 = F.frames([1, 0], gold, np.zeros((0, 2), np.float32), 1)
    d_out.fill_(np.uint32(SENTINEL).astype(np.int32).item())
    assert lib.dvbs2_plframer_frame_device(fr._h, None, 2, 1, d_out.data_ptr(), st) == capi.OK
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.array_equal(got[:want2.shape[0]], F.bits(want2)) and (got[want2.shape[0]:] == SENTINEL).all()
    refused(capi.EINVAL, "xfecframes is null and the framed prefix holds a data frame", lib.dvbs2_plframer_frame_device, fr._h, None, 3, -1,
            d_out.data_ptr(), st)
    fr.close()
