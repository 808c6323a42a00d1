"""The device encoder (dvbs2_enc_*, FecEncoder): BB scrambler -> BCH -> LDPC -> mapper, every comparison bit for bit.

BCH is pinned by the genuine reference encoder (oracle/_ref, RefBch) and the plain-C restatement, LDPC by the restated IRA encoder and by
the genuine reference DECODER's parity check: a word that passes H and carries the given information bits is THE codeword (the parity
part of H is invertible). The mapper is compared as uint32 views with the CPU mappers the other tests use."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import apsk_model
import demap_table_model as DT
import fec_testlib as T
from dvbs2rx_amd import (BchDecoder, Demapper, FecChain, FecEncoder, apsk_points, bb_descramble_sequence, capi, get_fec_info,
                         ldpc_table_info, ldpc_table_names)

pytestmark = pytest.mark.gpu

ROWS = json.load(open(os.path.join(T.ROOT, "tests", "golden", "fec_params.json")))["rows"]
BCH_CODES = T.bch_codes()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _messages(nf, nbytes, seed):
    """all zero, all one, a single 1 in the first and in the last position, the rest random"""
    m = np.random.default_rng(seed).integers(0, 256, (nf, nbytes), dtype=np.uint8)
    m[0] = 0
    if nf > 1:
        m[1] = 0xff
    if nf > 3:
        m[2] = 0; m[2, 0] = 0x80
        m[3] = 0; m[3, -1] = 0x01
    return m


def _row_ok(r, constellation=capi.ENC_NO_MAPPER):
    return capi.lib.dvbs2_enc_check(r["standard_id"], r["framesize_id"], r["rate_id"], constellation) == capi.OK


# ------------------------------------------------------------------ 1. BCH, every code
@pytest.mark.parametrize("row", BCH_CODES, ids=lambda r: "%s-n%d-t%d" % (r["framesize"][9:].lower(), r["bch_n"], r["bch_t"]))
def test_bch_every_code(row):
    """create_parts (BCH only) and, where the row allows it, create: n_frames 1, 31, 33 (the encoder has one path for every batch
    size) against RefBch.encode, OracleBch.encode_bytes, and back through dvbs2_bch_decode with 0 corrections."""
    m, prim = T.BCH_FIELDS[row["framesize_id"]]
    n, k, t = row["bch_n"], row["bch_k"], row["bch_t"]
    msg = _messages(33, k // 8, n)
    msg[4:8] = msg[0:4][::-1]  # (the four special words also behind each other in another order)
    ref = T.RefBch(prim, t, n)
    want = ref.encode(msg)
    ref.close()
    assert np.array_equal(want, T.OracleBch(m, prim, t, n).encode_bytes(msg))
    assert np.array_equal(want[:, :k // 8], msg)
    enc = FecEncoder.from_parts(bch=(m, prim, t, n), max_frames=33)
    assert (enc.in_bits, enc.bch_n, enc.ldpc_n, enc.n_syms, enc.n_mod) == (k, n, 0, 0, 0)
    for nf in (1, 31, 33):
        got = enc.work(msg[:nf])["bch_cw"]
        assert got.shape == (nf, n // 8) and np.array_equal(got, want[:nf]), nf
    enc.close()
    dec = BchDecoder(raw=(m, prim, t, n), max_frames=33)
    back, corr = dec.work(want)
    dec.close()
    assert np.array_equal(back, msg) and not corr.any()
    if _row_ok(row):
        enc = FecEncoder(row["standard_id"], row["framesize_id"], row["rate"], capi.ENC_NO_MAPPER, max_frames=33)
        assert (enc.in_bits, enc.bch_n, enc.ldpc_n, enc.n_syms, enc.n_mod) == (k, n, row["ldpc_n"], 0, 0)
        assert np.array_equal(enc.work(msg, want=["bch_cw"])["bch_cw"], want)
        enc.close()


def test_bch_rows_cover_create():
    assert sum(_row_ok(r) for r in BCH_CODES) > 30  # most codes also run through dvbs2_enc_create above


# ------------------------------------------------------------------ 2. BB scrambler
@pytest.mark.parametrize("framesize,rate", [(capi.FECFRAME_SHORT, "C1_4"), (capi.FECFRAME_NORMAL, "C9_10")])
def test_bb_scrambler(framesize, rate):
    fi = get_fec_info(capi.STANDARD_DVBS2, framesize, rate)
    kb = fi["bch_k"] // 8
    msg = _messages(5, kb, 77)
    enc = FecEncoder(capi.STANDARD_DVBS2, framesize, rate, capi.ENC_NO_MAPPER, max_frames=5)
    plain = enc.work(msg ^ bb_descramble_sequence(kb)[None, :])
    enc.set_scramble(True)
    scrambled = enc.work(msg)
    enc.set_scramble(False)
    off = enc.work(msg)
    enc.close()
    for name in ("bch_cw", "ldpc_cw"):
        assert np.array_equal(plain[name], scrambled[name]), name
        assert not np.array_equal(off[name], scrambled[name]), name
    assert np.array_equal(off["bch_cw"][:, :kb], msg)


# ------------------------------------------------------------------ 3. LDPC, every table
def _info_words(nf, K, seed):
    """all zero, all one, a single 1 at 0, 359, 360 and K - 1 (the rotation wrap, the first and the last group), the rest random"""
    b = np.random.default_rng(seed).integers(0, 2, (nf, K), dtype=np.uint8)
    if nf >= 6:
        b[0] = 0; b[1] = 1
        for f, pos in zip(range(2, 6), (0, 359, 360, K - 1)):
            b[f] = 0; b[f, pos] = 1
    return b


REF_DECODER_TABLES = {}  # one table of each family for the genuine reference decoder: filled below from the parameter rows


def _family(r):
    if r["table"].startswith("T2_"):
        return "T2"
    if r["framesize_id"] == capi.FECFRAME_MEDIUM:
        return "medium"
    if r["table"].startswith("S2X"):
        return "S2X"
    return "S2 normal" if r["framesize_id"] == capi.FECFRAME_NORMAL else "S2 short"


for _r in ROWS:
    REF_DECODER_TABLES.setdefault(_family(_r), _r["table"])


def test_ldpc_names_are_all_the_tables():
    names = ldpc_table_names()
    assert len(names) == 57 and set(REF_DECODER_TABLES) == {"S2 normal", "S2 short", "S2X", "T2", "medium"}
    assert set(REF_DECODER_TABLES.values()) <= set(names)


@pytest.mark.parametrize("table", ldpc_table_names())
def test_ldpc_every_table(table):
    """create_parts (LDPC only), 33 frames (crosses 32): equal to the restated IRA encoder; for one table of each family the genuine
    reference decoder (generic) converges on +-100 LLRs of the device codeword and returns the same bits."""
    ti = ldpc_table_info(table)
    N, K = ti["N"], ti["K"]
    info = _info_words(33, K, N + K)
    enc = FecEncoder.from_parts(ldpc_table=table, max_frames=33)
    assert (enc.in_bits, enc.bch_n, enc.ldpc_n, enc.n_syms) == (K, 0, N, 0)
    got = enc.work(np.packbits(info, axis=1))["ldpc_cw"]
    enc.close()
    bits = np.unpackbits(got, axis=1)
    assert bits.shape == (33, N) and np.array_equal(bits[:, :K], info)
    assert np.array_equal(bits, T.ldpc_encode(table, info))
    if table in REF_DECODER_TABLES.values():
        assert T.ref_ldpc() is not None, "oracle/_ref/libdvbs2_ref_ldpc.so absent"
        llr = (100 * (1 - 2 * bits[:16].astype(np.int16))).astype(np.int8)
        out, rets = T.ref_ldpc_decode(table, llr, 2, 5)
        assert all(r >= 0 for r in rets), rets
        assert np.array_equal((out < 0).astype(np.uint8), bits[:16])


@pytest.mark.parametrize("table", ["S2_TABLE_C1", "S2_TABLE_B4"])
@pytest.mark.parametrize("nf", [1, 32, 65])
def test_ldpc_batch_sizes(table, nf):
    ti = ldpc_table_info(table)
    info = _info_words(nf, ti["K"], nf)
    enc = FecEncoder.from_parts(ldpc_table=table, max_frames=65)
    got = np.unpackbits(enc.work(np.packbits(info, axis=1))["ldpc_cw"], axis=1)
    enc.close()
    assert np.array_equal(got, T.ldpc_encode(table, info))


# ------------------------------------------------------------------ 4. mapper, every form
def _first_row(pred, constellation):
    """the first DVB-S2 row that satisfies pred and takes the constellation, short frames before the others"""
    rows = [r for r in ROWS if r["standard_id"] == capi.STANDARD_DVBS2 and pred(r) and _row_ok(r, constellation)]
    rows.sort(key=lambda r: r["framesize_id"] != capi.FECFRAME_SHORT)
    assert rows
    return rows[0]


def _mapper_cases():
    yield "qpsk", capi.MOD_QPSK, _first_row(lambda r: r["rate"] == "C1_4", capi.MOD_QPSK)
    for order in (0, 1, 2):
        yield "8psk-order%d" % order, capi.MOD_8PSK, _first_row(lambda r: T.column_order(r["rate"]) == order, capi.MOD_8PSK)
    yield "16apsk", capi.MOD_16APSK, _first_row(lambda r: True, capi.MOD_16APSK)
    yield "32apsk", capi.MOD_32APSK, _first_row(lambda r: True, capi.MOD_32APSK)
    for name in ("qam64", "qam256"):
        yield name, name, _first_row(lambda r: r["rate"] == "C3_4", capi.ENC_NO_MAPPER)


MAPPER_CASES = list(_mapper_cases())


def _wrong_signs(llr, bits):
    """LLRs whose sign spells the other bit (a zero LLR spells nothing)"""
    return int((((llr < 0) & (bits == 0)) | ((llr > 0) & (bits == 1))).sum())


@pytest.mark.parametrize("name,constellation,row", MAPPER_CASES, ids=[c[0] for c in MAPPER_CASES])
def test_mapper_every_form(name, constellation, row):
    """Three frames; the symbols as uint32 views against the CPU mapper of the form, and the demapper's signs at N0 = 0.1 spell the
    codeword bits. (At N0 = 0.1 the nearest neighbours of the 256-point table are 0.235 LLR units apart, which the demapper's int8
    rounds to 0 for ANY mapper: there no LLR may have the wrong sign, and the signs spell every bit at N0 = 0.01.)"""
    fs, rate = row["framesize_id"], row["rate"]
    kb = row["bch_k"] // 8
    msg = _messages(3, kb, 4000 + len(name))
    if isinstance(constellation, str):
        n_mod, column, _ = DT.E2E[name]
        pts = DT.gray_qam(n_mod).astype(np.complex64)
        assert list(column) != list(range(n_mod))
        enc = FecEncoder.from_table(capi.STANDARD_DVBS2, fs, rate, pts, column, max_frames=3)
        dm = Demapper.from_table(fs, pts, column, max_frames=3)
    else:
        enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, constellation, max_frames=3)
        dm = Demapper(fs, rate, constellation, max_frames=3)
    out = enc.work(msg)
    assert (enc.n_syms, enc.n_mod) == (dm.n_syms, dm.n_mod) and enc.n_syms * enc.n_mod == row["ldpc_n"]
    enc.close()
    cw = np.unpackbits(out["ldpc_cw"], axis=1)
    if isinstance(constellation, str):
        want = DT.map_bits_columns(cw, pts, column)
    elif constellation == capi.MOD_QPSK:
        want = ((1 - 2.0 * cw[:, 0::2]) + 1j * (1 - 2.0 * cw[:, 1::2])) * np.sqrt(0.5)
    elif constellation == capi.MOD_8PSK:
        order = T.column_order(rate)
        assert order == dm.column_order and order == int(name[-1])
        rows = cw.shape[1] // 3
        want = T.map_8psk(np.stack([cw[:, a:a + rows] for a in T.column_bases(rows, order)], axis=-1))
    else:
        want = apsk_model.map_bits(cw, apsk_points(constellation, rate))
    want = np.ascontiguousarray(want).astype(np.complex64)
    syms = out["syms"]
    assert syms.dtype == np.complex64 and syms.shape == want.shape
    assert np.array_equal(syms.view(np.uint32), want.view(np.uint32))
    llr = dm.work(syms, np.float32(0.1))
    assert _wrong_signs(llr, cw) == 0
    if name == "qam256":
        llr = dm.work(syms, np.float32(0.01))
    dm.close()
    assert np.array_equal((llr < 0).astype(np.uint8), cw) and (llr != 0).all()


APSK_ROWS = [(mod, rate, fs) for mod, rates in ((capi.MOD_16APSK, apsk_model.GAMMA_16), (capi.MOD_32APSK, apsk_model.GAMMA_32))
             for rate in rates for fs in ((capi.FECFRAME_NORMAL,) if rate == "C9_10" else (capi.FECFRAME_NORMAL, capi.FECFRAME_SHORT))]


@pytest.mark.parametrize("constellation,rate,fs", APSK_ROWS, ids=["%dapsk-%s-%s" % (len(apsk_model.ring_angle(m)), r, "short" if f == capi.FECFRAME_SHORT else "normal")
                                                                  for m, r, f in APSK_ROWS])
def test_mapper_every_apsk_rate(constellation, rate, fs):
    """Every legal (constellation, rate, frame size) of MODCODs 18-28, three frames: the symbols as uint32 views against the model's
    mapper on the rate's own table (the ring ratios differ from rate to rate), and the demapper of the same rate at N0 = 0.01
    spells every codeword bit."""
    row = next(r for r in ROWS if r["standard_id"] == capi.STANDARD_DVBS2 and r["framesize_id"] == fs and r["rate"] == rate)
    msg = _messages(3, row["bch_k"] // 8, 4100 + row["rate_id"])
    enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, constellation, max_frames=3)
    dm = Demapper(fs, rate, constellation, max_frames=3)
    out = enc.work(msg)
    assert (enc.n_syms, enc.n_mod) == (dm.n_syms, dm.n_mod) and enc.n_syms * enc.n_mod == row["ldpc_n"]
    enc.close()
    cw = np.unpackbits(out["ldpc_cw"], axis=1)
    want = np.ascontiguousarray(apsk_model.map_bits(cw, apsk_points(constellation, rate))).astype(np.complex64)
    syms = out["syms"]
    assert syms.dtype == np.complex64 and syms.shape == want.shape
    assert np.array_equal(syms.view(np.uint32), want.view(np.uint32))
    assert np.allclose(want, apsk_model.map_bits(cw, apsk_model.points(constellation, rate)), rtol=0, atol=1e-6)  # the library's table is the rate's
    llr = dm.work(syms, np.float32(0.01))
    dm.close()
    assert np.array_equal((llr < 0).astype(np.uint8), cw) and (llr != 0).all()


# ------------------------------------------------------------------ 5. all outputs at once equal each alone; a null output is not written
GUARD = 64


class _Guarded:
    """a device buffer between two guards of GUARD bytes"""

    def __init__(self, nbytes, fill=0xA5):
        import torch
        self.fill, self.nbytes = fill, nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda:0")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def body(self):
        return self.t[GUARD:GUARD + self.nbytes].cpu().numpy()

    def guards_intact(self):
        g = self.t.cpu().numpy()
        return (g[:GUARD] == self.fill).all() and (g[GUARD + self.nbytes:] == self.fill).all()

    def untouched(self):
        return (self.t.cpu().numpy() == self.fill).all()


def test_outputs_together_and_alone():
    import torch
    fs, rate, nf = capi.FECFRAME_SHORT, "C3_5", 5
    enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, capi.MOD_8PSK, max_frames=nf)
    sizes = (nf * enc.bch_n // 8, nf * enc.ldpc_n // 8, nf * enc.n_syms * 8)
    msg = _messages(nf, enc.in_bytes, 5)
    d_in = _dev(msg)
    allb = [_Guarded(s) for s in sizes]
    enc.work_device(d_in.data_ptr(), nf, *[b.ptr for b in allb])
    torch.cuda.synchronize()
    assert all(b.guards_intact() for b in allb)
    together = [b.body() for b in allb]
    host = enc.work(msg)
    assert np.array_equal(together[0], host["bch_cw"].reshape(-1)) and np.array_equal(together[1], host["ldpc_cw"].reshape(-1))
    assert np.array_equal(together[2].view(np.uint32), host["syms"].reshape(-1).view(np.uint32))
    for i in range(3):
        bufs = [_Guarded(s) for s in sizes]
        ptrs = [b.ptr if j == i else 0 for j, b in enumerate(bufs)]
        enc.work_device(d_in.data_ptr(), nf, *ptrs)
        torch.cuda.synchronize()
        assert bufs[i].guards_intact() and np.array_equal(bufs[i].body(), together[i]), i
        assert all(bufs[j].untouched() for j in range(3) if j != i), i  # what nobody asked for is not written
        # ... not even into what an earlier call was given
        assert all(np.array_equal(allb[j].body(), together[j]) and allb[j].guards_intact() for j in range(3))
    enc.close()


# ------------------------------------------------------------------ 6. loopback on the device
def _bbframes(kbch, nf, seed):
    rng = np.random.default_rng(seed)
    dfl = (kbch - 80) // 8
    return T.bbframe_stream(kbch, nf, T.ts_up_stream(nf * dfl // 188 + 2, rng))


LOOPBACK = [("qpsk-1/4-short", capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK, 40), ("8psk-3/5-short", capi.FECFRAME_SHORT, "C3_5", capi.MOD_8PSK, 40),
            ("16apsk-2/3-short", capi.FECFRAME_SHORT, "C2_3", capi.MOD_16APSK, 40), ("32apsk-3/4-short", capi.FECFRAME_SHORT, "C3_4", capi.MOD_32APSK, 40),
            ("qam64-3/4-short", capi.FECFRAME_SHORT, "C3_4", "qam64", 40), ("qpsk-1/2-normal", capi.FECFRAME_NORMAL, "C1_2", capi.MOD_QPSK, 33)]


@pytest.mark.parametrize("name,fs,rate,constellation,nf", LOOPBACK, ids=[c[0] for c in LOOPBACK])
def test_loopback_on_the_device(name, fs, rate, constellation, nf):
    """Random BBFRAMEs -> FecEncoder (scramble on) -> symbols that stay on the device -> FecChain.work_device (descramble on): the
    same bytes, every LDPC group converged, no BCH correction."""
    import torch
    fi = get_fec_info(capi.STANDARD_DVBS2, fs, rate)
    frames = _bbframes(fi["bch_k"], nf, 900 + nf + len(name))
    assert frames.shape == (nf, fi["bch_k"] // 8)
    if isinstance(constellation, str):
        n_mod, column, _ = DT.E2E[constellation]
        pts = DT.gray_qam(n_mod).astype(np.complex64)
        enc = FecEncoder.from_table(capi.STANDARD_DVBS2, fs, rate, pts, column, max_frames=nf)
        chain = FecChain.from_table(capi.STANDARD_DVBS2, fs, rate, pts, column, group_size=32, max_frames=nf)
    else:
        enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, constellation, max_frames=nf)
        chain = FecChain(capi.STANDARD_DVBS2, fs, rate, constellation, group_size=32, max_frames=nf)
    enc.set_scramble(True)
    chain.set_descramble(True)
    assert enc.n_syms == chain.n_syms and enc.in_bytes == chain.msg_bytes
    d_in = _dev(frames)
    d_syms = torch.zeros((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda:0")
    d_n0 = torch.full((1,), 0.02, dtype=torch.float32, device="cuda:0")
    d_msg = torch.zeros((nf, chain.msg_bytes), dtype=torch.uint8, device="cuda:0")
    d_ret = torch.full(((nf + 31) // 32,), -7, dtype=torch.int32, device="cuda:0")
    d_corr = torch.full((nf,), -7, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    enc.work_device(d_in.data_ptr(), nf, d_syms=d_syms.data_ptr(), stream=stream)
    chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr(), stream)
    torch.cuda.synchronize()
    ret, corr = d_ret.cpu().numpy(), d_corr.cpu().numpy()
    enc.close(); chain.close()
    assert (ret >= 0).all(), ret
    assert (corr == 0).all(), corr
    assert np.array_equal(d_msg.cpu().numpy(), frames)


# ------------------------------------------------------------------ 7. asynchrony and placement
def test_async_calls_and_placement():
    import torch
    fs, rate, nf = capi.FECFRAME_SHORT, "C1_4", 6
    enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, capi.MOD_QPSK, max_frames=nf)
    a, b = _messages(nf, enc.in_bytes, 1), _messages(nf, enc.in_bytes, 2)[::-1].copy()
    want = [enc.work(x) for x in (a, b)]  # separate, synchronous calls through the host entry
    d = [_dev(x) for x in (a, b)]

    def outputs():
        return [(torch.zeros((nf, enc.bch_n // 8), dtype=torch.uint8, device="cuda:0"), torch.zeros((nf, enc.ldpc_n // 8), dtype=torch.uint8, device="cuda:0"),
                 torch.zeros((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda:0")) for _ in range(2)]

    def same(outs):
        for o, w in zip(outs, want):
            assert np.array_equal(o[0].cpu().numpy(), w["bch_cw"]) and np.array_equal(o[1].cpu().numpy(), w["ldpc_cw"])
            assert np.array_equal(o[2].cpu().numpy().view(np.uint32).reshape(nf, -1), w["syms"].view(np.uint32))

    torch.cuda.synchronize()
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        outs = outputs()
        torch.cuda.synchronize()
        for x, o in zip(d, outs):  # two calls behind each other, no host wait in between
            enc.work_device(x.data_ptr(), nf, *[t.data_ptr() for t in o], stream=stream.cuda_stream)
        stream.synchronize()
        same(outs)
    # the device entry with single outputs equals the host entry, too
    o = outputs()[0]
    enc.work_device(d[0].data_ptr(), nf, d_syms=o[2].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(o[2].cpu().numpy().view(np.uint32).reshape(nf, -1), want[0]["syms"].view(np.uint32))
    # in place (d_in inside d_bch_cw) is refused: the frames of input and output have different strides
    big = torch.zeros((nf * enc.bch_n // 8,), dtype=torch.uint8, device="cuda:0")
    big[:nf * enc.in_bytes] = d[0].reshape(-1)
    torch.cuda.synchronize()
    with pytest.raises(capi.Dvbs2Error) as e:
        enc.work_device(big.data_ptr(), nf, d_bch_cw=big.data_ptr())
    assert e.value.code == capi.EINVAL and "d_in overlaps an output: encoding in place is not supported" in str(e.value)
    assert np.array_equal(big[:nf * enc.in_bytes].cpu().numpy(), a.reshape(-1))
    # n_frames 0 is a no-op, max_frames + 1 is DVBS2_ESIZE
    g = _Guarded(64)
    enc.work_device(d[0].data_ptr(), 0, d_bch_cw=g.ptr)
    enc.work_device(0, 0)
    assert enc.work(a[:0]) and all(v.shape[0] == 0 for v in enc.work(a[:0]).values())
    torch.cuda.synchronize()
    assert g.untouched()
    for call in (lambda: enc.work_device(d[0].data_ptr(), nf + 1, d_bch_cw=g.ptr), lambda: enc.work(np.zeros((nf + 1, enc.in_bytes), np.uint8))):
        with pytest.raises(capi.Dvbs2Error) as e:
            call()
        assert e.value.code == capi.ESIZE and "n_frames exceeds max_frames" in str(e.value)
    torch.cuda.synchronize()
    assert g.untouched()
    enc.close()


# ------------------------------------------------------------------ 8. error texts
def test_error_texts():
    import torch
    lib, h = capi.lib, C.c_void_p()
    m, prim = T.BCH_FIELDS[capi.FECFRAME_SHORT]
    # creation, with a device present
    T.refused(capi.EINVAL, "max_frames must be in 1..65535 (frames are one launch dimension)", lib.dvbs2_enc_create, C.byref(h), 0, 0, 0, capi.MOD_QPSK, 0, 0)
    T.refused(capi.EINVAL, "device index out of range", lib.dvbs2_enc_create, C.byref(h), 0, 0, 0, capi.MOD_QPSK, 4, 99)
    T.refused(capi.EINVAL, "bch_n 3240 != table K 5400 of S2_TABLE_C2", lib.dvbs2_enc_create_parts, C.byref(h), m, prim, 12, 3240, b"S2_TABLE_C2", 4, 0)
    T.refused(capi.EINVAL, "Codeword length n exceeds the maximum of (2^m - 1)", lib.dvbs2_enc_create_parts, C.byref(h), m, prim, 12, 20000, None, 4, 0)
    T.refused(capi.EINVAL, "u8 array messages are only supported for n and k multiple of 8.", lib.dvbs2_enc_create_parts, C.byref(h), m, prim, 12, 3241, None, 4, 0)
    assert lib.dvbs2_enc_create(C.byref(h), 0, 1, 3, capi.MOD_16APSK, 4, 0) == capi.EINVAL
    assert lib.dvbs2_last_error().startswith(b"constellation: Unsupported code rate for 16APSK / 32APSK")
    t2 = next(r for r in ROWS if r["standard_id"] == capi.STANDARD_DVBT2 and _row_ok(r))
    assert lib.dvbs2_enc_create(C.byref(h), t2["standard_id"], t2["framesize_id"], t2["rate_id"], capi.MOD_QPSK, 4, 0) == capi.EINVAL
    assert lib.dvbs2_last_error().startswith(b"constellation: a DVB-T2 rate has no built-in mapper")
    # ... where DVBS2_ENC_NO_MAPPER and a caller's table are accepted
    pts = DT.gray_qam(6).astype(np.complex64)
    for make in (lambda: FecEncoder(t2["standard_id"], t2["framesize_id"], t2["rate"], capi.ENC_NO_MAPPER, max_frames=2),
                 lambda: FecEncoder.from_table(t2["standard_id"], t2["framesize_id"], t2["rate"], pts, None, max_frames=2)):
        e = make()
        assert e.ldpc_n == t2["ldpc_n"]
        e.close()
    # calls
    full = FecEncoder(capi.STANDARD_DVBS2, capi.FECFRAME_SHORT, "C1_4", capi.ENC_NO_MAPPER, max_frames=2)
    bch = FecEncoder.from_parts(bch=(m, prim, 12, 3240), max_frames=2)
    ldpc = FecEncoder.from_parts(ldpc_table="S2_TABLE_C1", max_frames=2)
    buf = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda:0")
    p, q = buf.data_ptr(), buf.data_ptr() + (1 << 15)
    host = np.zeros(1 << 15, np.uint8)
    hp = host.ctypes.data
    for n in (1, 0):  # an absent stage is refused whatever n_frames is
        T.refused(capi.EINVAL, "d_syms: this encoder has no mapper", lib.dvbs2_enc_encode_device, full._h, p, n, None, None, q, None)
        T.refused(capi.EINVAL, "d_ldpc_cw: this encoder has no LDPC stage", lib.dvbs2_enc_encode_device, bch._h, p, n, None, q, None, None)
        T.refused(capi.EINVAL, "d_bch_cw: this encoder has no BCH stage", lib.dvbs2_enc_encode_device, ldpc._h, p, n, q, None, None, None)
        T.refused(capi.EINVAL, "d_bch_cw: this encoder has no BCH stage", lib.dvbs2_enc_encode, ldpc._h, hp, n, hp, None, None)
    T.refused(capi.EINVAL, "no output requested", lib.dvbs2_enc_encode_device, full._h, p, 1, None, None, None, None)
    T.refused(capi.EINVAL, "no output requested", lib.dvbs2_enc_encode, full._h, hp, 1, None, None, None)
    T.refused(capi.EINVAL, "d_in is NULL", lib.dvbs2_enc_encode_device, full._h, None, 1, q, None, None, None)
    T.refused(capi.EINVAL, "d_in is NULL", lib.dvbs2_enc_encode, full._h, None, 1, hp, None, None)
    T.refused(capi.EINVAL, "bad argument", lib.dvbs2_enc_encode_device, full._h, p, -1, q, None, None, None)
    T.refused(capi.ESIZE, "n_frames exceeds max_frames", lib.dvbs2_enc_encode_device, full._h, p, 3, q, None, None, None)
    T.refused(capi.EINVAL, "d_in overlaps an output: encoding in place is not supported", lib.dvbs2_enc_encode_device, full._h, p, 2, None, p + 100, None, None)
    T.refused(capi.EINVAL, "no BCH stage: the BB scrambler is part of its load", lib.dvbs2_enc_set_scramble, ldpc._h, 1)
    # a refused call leaves the handle usable
    assert lib.dvbs2_enc_encode_device(full._h, p, 2, q, None, None, None) == capi.OK
    torch.cuda.synchronize()
    for e in (full, bch, ldpc):
        e.close()
