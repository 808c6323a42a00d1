"""The device BB framer (dvbs2_bbframer_*, BbFramer): TS packets -> BBFRAMEs, every comparison byte for byte against the numpy model
(tests/bbframer_model.py, pinned on the CPU by tests/test_bbframer_model.py), then into the device de-header and round the closed loop
encoder -> decoder chain -> de-header. The null-handle answers of the new entries need no device: tests/test_bbframer_host.py."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
from bbframer_model import TS, BbFramerModel, expected_packets
from dvbs2rx_amd import BbDeheader, BbFramer, FecChain, FecEncoder, capi, get_fec_info

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 64


def _dfls(kbch):
    mx = kbch // 8 - 10
    return [0, mx // TS * TS, 188, 189, mx - 5]


def _dev_at(a, off):
    """a copy of `a` on the device that starts `off` bytes behind a 16-byte boundary"""
    import torch
    base = torch.zeros(a.size + 32, dtype=torch.uint8, device="cuda:0")
    assert base.data_ptr() % 16 == 0
    view = base[off:off + a.size]
    view.copy_(torch.from_numpy(np.array(a, np.uint8).reshape(-1)))
    return view


def _run(fr, ts, n_frames, dfl, in_off=0, out_off=0):
    """One work_device call; returns the frames after checking everything around them: the sentinels in front of and behind the output,
    the input unchanged."""
    import torch
    need = fr.need(n_frames, dfl)
    src = np.array(ts[:need * TS], np.uint8)
    d_in = _dev_at(src, in_off)
    total = n_frames * fr.kbch_bytes
    d_out = torch.full((out_off + total + PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    assert d_out.data_ptr() % 16 == 0
    fr.work_device(d_in.data_ptr(), n_frames, d_out.data_ptr() + out_off, dfl, T.stream())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:out_off] == SENTINEL).all() and (out[out_off + total:] == SENTINEL).all(), "wrote outside the frames"
    assert np.array_equal(d_in.cpu().numpy(), src), "input changed"
    return out[out_off:out_off + total].reshape(n_frames, fr.kbch_bytes), need


_REF = {}


def _reference(kbch, dfl, n_frames=33):
    """(packets, frames) of the model from pos = 0, computed once and read-only; a shorter call from pos = 0 is a prefix of it."""
    key = (kbch, dfl, n_frames)
    if key not in _REF:
        m = BbFramerModel(kbch)
        ups = T.ts_up_stream(m.need(n_frames, dfl), np.random.default_rng(kbch + dfl))
        frames = m.work(ups, n_frames, dfl)
        ups.setflags(write=False)
        frames.setflags(write=False)
        _REF[key] = (ups, frames)
    return _REF[key]


# ------------------------------------------------------------------ 1. every byte against the model
@pytest.mark.parametrize("kbch", (3072, 16008, 58192))
@pytest.mark.parametrize("dfl_index", range(5), ids=("max", "whole-packets", "188", "189", "max-5"))
def test_every_byte(kbch, dfl_index):
    dfl = _dfls(kbch)[dfl_index]
    ups, want = _reference(kbch, dfl)
    eff = dfl or kbch // 8 - 10
    fr = BbFramer(kbch_bits=kbch, max_frames=33)
    assert (fr.kbch_bytes, fr.max_dfl_bytes, fr.max_packets_per_call) == (kbch // 8, kbch // 8 - 10, -(-33 * (kbch // 8 - 10) // TS))
    for n in (1, 2, 7, 33):
        for in_off in (0, 1, 3):
            for out_off in (0, 1):
                fr.reset(T.stream())
                got, need = _run(fr, ups, n, dfl, in_off, out_off)
                assert need == -(-n * eff // TS)
                assert np.array_equal(got, want[:n]), (n, in_off, out_off)
                assert (got[:, 10 + eff:] == 0).all()
                assert fr.counters(T.stream()) == dict(packets=need, bbframes=n, sync_errors=0)
    fr.close()


def test_matype():
    kbch = 16008
    m = BbFramerModel(kbch)
    m.set_matype(0xF1, 0x2A)
    ups = T.ts_up_stream(m.need(5), np.random.default_rng(3))
    want = m.work(ups, 5)
    fr = BbFramer(kbch_bits=kbch, max_frames=8)
    fr.set_matype(0xF1, 0x2A)
    got, _ = _run(fr, ups, 5, 0)
    assert np.array_equal(got, want) and got[0, 0] == 0xF1 and got[4, 1] == 0x2A
    fr.close()


def test_wrong_sync_bytes_are_framed_and_counted():
    kbch = 3072
    m = BbFramerModel(kbch)
    ups = T.ts_up_stream(m.need(7), np.random.default_rng(4))
    ups[0], ups[TS], ups[-TS] = 0x12, 0x34, 0x56
    want = m.work(ups, 7)
    fr = BbFramer(kbch_bits=kbch, max_frames=8)
    got, need = _run(fr, ups, 7, 0, in_off=1)
    assert np.array_equal(got, want) and got[0, 10] == 0x12
    assert fr.counters(T.stream()) == m.counters() == dict(packets=need, bbframes=7, sync_errors=3)
    fr.close()


# ------------------------------------------------------------------ 2. the carry
def test_carry_walks_every_residue():
    """190 calls of one frame with dfl_bytes = 189: pos mod 188 takes every value, 0 (a finished CRC is carried) and 187 among them."""
    kbch, n = 3072, 190
    ups, want = _reference(kbch, 189, n)
    fr = BbFramer(kbch_bits=kbch, max_frames=n)
    m = BbFramerModel(kbch)
    pk, seen = 0, set()
    for f in range(n):
        seen.add(m.pos % TS)
        need = m.need(1, 189)
        assert fr.need(1, 189) == need
        got, _ = _run(fr, ups[pk * TS:], 1, 189, in_off=f % 4)
        assert np.array_equal(got, m.work(ups[pk * TS:], 1, 189)) and np.array_equal(got[0], want[f]), f
        pk += need
    assert seen == set(range(TS)) and pk * TS == ups.size
    assert fr.counters(T.stream()) == m.counters()
    fr.reset(T.stream())
    got, _ = _run(fr, ups, n, 189)
    assert np.array_equal(got, want)
    fr.close()


def test_random_calls_with_changing_dfl_and_reset():
    kbch = 16008
    rng = np.random.default_rng(8)
    ups = T.ts_up_stream(300 * (kbch // 8) // TS + 2, rng)
    fr = BbFramer(kbch_bits=kbch, max_frames=32)
    for part in range(2):  # the second part after a reset in the middle of a packet: a fresh handle
        m = BbFramerModel(kbch)
        pk, f, total = 0, 0, 150 if part else 300
        while f < total:
            n, dfl = min(int(rng.integers(0, 33)), total - f), int(rng.choice(_dfls(kbch)))
            need = m.need(n, dfl)
            assert fr.need(n, dfl) == need
            want = m.work(ups[pk * TS:], n, dfl)
            if n == 0:
                fr.work_device(0, 0, 0, dfl, T.stream())  # a valid call that changes nothing
            else:
                got, _ = _run(fr, ups[pk * TS:], n, dfl, in_off=int(rng.integers(0, 4)), out_off=int(rng.integers(0, 2)))
                assert np.array_equal(got, want), (part, f, n, dfl)
            pk += need
            f += n
        dfl = 189 if (m.pos + 189) % TS else 190  # leave the stream inside a packet
        got, _ = _run(fr, ups[pk * TS:], 1, dfl)
        assert np.array_equal(got, m.work(ups[pk * TS:], 1, dfl)) and m.pos % TS != 0
        assert fr.counters(T.stream()) == m.counters()
        fr.reset(T.stream())
        assert fr.counters(T.stream()) == dict(packets=0, bbframes=0, sync_errors=0) and fr.need(1, 188) == 1
    fr.close()


# ------------------------------------------------------------------ 3. into the device de-header
@pytest.mark.parametrize("kbch", (7032, 58192))
@pytest.mark.parametrize("whole_packets", (False, True), ids=("dfl-max", "dfl-whole-packets"))
def test_into_the_device_deheader(kbch, whole_packets):
    import torch
    mx = kbch // 8 - 10
    dfl = mx // TS * TS if whole_packets else 0
    total = 64 * (dfl or mx)
    ups = T.ts_up_stream(-(-total // TS), np.random.default_rng(kbch))
    fr, dh = BbFramer(kbch_bits=kbch, max_frames=64), BbDeheader(kbch_bits=kbch, max_frames=64)
    st = T.stream()
    d_ts = _dev_at(ups, 0)
    d_bb = torch.zeros((64, kbch // 8), dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(64 * dh.max_out_bytes_per_frame, dtype=torch.uint8, device="cuda:0")
    n1 = fr.need(40, dfl)
    fr.work_device(d_ts.data_ptr(), 40, d_bb.data_ptr(), dfl, st)
    assert n1 + fr.need(24, dfl) == ups.size // TS
    fr.work_device(d_ts.data_ptr() + n1 * TS, 24, d_bb[40].data_ptr(), dfl, st)
    dh.work_device(d_bb.data_ptr(), 40, d_out.data_ptr(), st)
    p1 = dh.finish(st)
    dh.work_device(d_bb[40].data_ptr(), 24, d_out.data_ptr() + p1, st)
    p2 = dh.finish(st)
    n = expected_packets(total)
    assert p1 + p2 == n * TS and np.array_equal(d_out[:p1 + p2].cpu().numpy(), ups[:n * TS])
    c = dh.counters(st)
    assert c["errors"] == c["gaps"] == c["dropped"] == c["overruns"] == 0 and c["bbframes"] == 64 and c["packets"] == n
    assert fr.counters(st) == dict(packets=ups.size // TS, bbframes=64, sync_errors=0)
    fr.close(); dh.close()


# ------------------------------------------------------------------ 4. the closed loop
@pytest.mark.parametrize("rate,constellation", (("C1_4", capi.MOD_QPSK), ("C3_5", capi.MOD_8PSK)), ids=("qpsk-1/4-short", "8psk-3/5-short"))
def test_closed_loop_on_the_device(rate, constellation):
    """TS packets -> BbFramer -> FecEncoder (scramble on) -> noise-free symbols -> FecChain (descramble on) -> BbDeheader -> the TS
    packets, nothing copied to the host in between."""
    import torch
    fs, nf = capi.FECFRAME_SHORT, 40
    kbch = get_fec_info(capi.STANDARD_DVBS2, fs, rate)["bch_k"]
    fr = BbFramer(capi.STANDARD_DVBS2, fs, rate, max_frames=nf)
    enc = FecEncoder(capi.STANDARD_DVBS2, fs, rate, constellation, max_frames=nf)
    chain = FecChain(capi.STANDARD_DVBS2, fs, rate, constellation, group_size=32, max_frames=nf)
    dh = BbDeheader(capi.STANDARD_DVBS2, fs, rate, max_frames=nf)
    enc.set_scramble(True)
    chain.set_descramble(True)
    assert fr.kbch_bytes == enc.in_bytes == chain.msg_bytes == dh.kbch_bytes == kbch // 8
    ups = T.ts_up_stream(fr.need(nf), np.random.default_rng(kbch))
    st = T.stream()
    d_ts = _dev_at(ups, 0)
    d_bb = torch.zeros((nf, fr.kbch_bytes), dtype=torch.uint8, device="cuda:0")
    d_syms = torch.zeros((nf, enc.n_syms, 2), dtype=torch.float32, device="cuda:0")
    d_n0 = torch.full((1,), 0.02, dtype=torch.float32, device="cuda:0")
    d_msg = torch.zeros((nf, chain.msg_bytes), dtype=torch.uint8, device="cuda:0")
    d_ret = torch.full(((nf + 31) // 32,), -7, dtype=torch.int32, device="cuda:0")
    d_corr = torch.full((nf,), -7, dtype=torch.int32, device="cuda:0")
    d_out = torch.zeros(nf * dh.max_out_bytes_per_frame, dtype=torch.uint8, device="cuda:0")
    fr.work_device(d_ts.data_ptr(), nf, d_bb.data_ptr(), 0, st)
    enc.work_device(d_bb.data_ptr(), nf, d_syms=d_syms.data_ptr(), stream=st)
    chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), 1, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr(), st)
    dh.work_device(d_msg.data_ptr(), nf, d_out.data_ptr(), st)
    produced = dh.finish(st)
    ret, corr = d_ret.cpu().numpy(), d_corr.cpu().numpy()
    assert (ret >= 0).all(), ret
    assert (corr == 0).all(), corr
    n = expected_packets(nf * fr.max_dfl_bytes)
    assert produced == n * TS and np.array_equal(d_out[:produced].cpu().numpy(), ups[:n * TS])
    assert np.array_equal(d_msg.cpu().numpy(), d_bb.cpu().numpy())
    c = dh.counters(st)
    assert c["errors"] == c["gaps"] == c["dropped"] == 0 and c["bbframes"] == nf
    for o in (fr, enc, chain, dh):
        o.close()


# ------------------------------------------------------------------ 5. host entry and errors
def test_host_entry_equals_device_entry():
    kbch = 16008
    ups, want = _reference(kbch, 189)
    fr = BbFramer(kbch_bits=kbch, max_frames=33)
    for n0, n1 in ((0, 7), (7, 7), (7, 33)):  # an empty call, a first call, a call that starts inside a packet
        need = fr.need(n1 - n0, 189)
        pk = -(-n0 * 189 // TS)
        got = fr.work(ups[pk * TS:], n1 - n0, 189)
        assert fr.packets_read == need and np.array_equal(got, want[n0:n1])
    fr.close()


def _refused(code, word, call, *args, **kwargs):
    with pytest.raises(capi.Dvbs2Error) as e:
        call(*args, **kwargs)
    assert e.value.code == code and word in capi.lib.dvbs2_last_error().decode(), (e.value, word)


def test_refusals_leave_the_handle_as_it_was():
    import torch
    kbch = 3072
    mx = kbch // 8 - 10
    ups, want = _reference(kbch, 189, 190)
    for bad_kbch, word in ((1576, "kbch_bits"), (65616, "kbch_bits"), (3073, "kbch_bits")):
        _refused(capi.EINVAL, word, BbFramer, kbch_bits=bad_kbch, max_frames=8)
    for bad_mf in (0, 65536):
        _refused(capi.EINVAL, "max_frames", BbFramer, kbch_bits=kbch, max_frames=bad_mf)
    fr = BbFramer(kbch_bits=kbch, max_frames=8)
    got, need = _run(fr, ups, 3, 189)  # pos = 567: inside a packet
    assert np.array_equal(got, want[:3])
    before = fr.counters(T.stream())
    d_in = _dev_at(ups[need * TS:], 0)
    d_out = torch.full((8 * fr.kbch_bytes,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    st = T.stream()
    for dfl in (187, mx + 1, -1):
        _refused(capi.EINVAL, "dfl_bytes", fr.work_device, d_in.data_ptr(), 1, d_out.data_ptr(), dfl, st)
        _refused(capi.EINVAL, "dfl_bytes", fr.need, 1, dfl)
        _refused(capi.EINVAL, "dfl_bytes", fr.work, ups, 1, dfl)
    for n in (-1, 9):
        _refused(capi.ESIZE, "n_frames", fr.work_device, d_in.data_ptr(), n, d_out.data_ptr(), 189, st)
        _refused(capi.ESIZE, "n_frames", fr.need, n, 189)
    _refused(capi.EINVAL, "matype1", fr.set_matype, 256, 0)
    _refused(capi.EINVAL, "matype2", fr.set_matype, 0xF2, -1)
    _refused(capi.EINVAL, "d_ts", fr.work_device, 0, 1, d_out.data_ptr(), 189, st)
    _refused(capi.EINVAL, "d_bbframes", fr.work_device, d_in.data_ptr(), 1, 0, 189, st)
    # ranges that overlap: the output begins inside the input, the input begins inside the output
    _refused(capi.EINVAL, "overlap", fr.work_device, d_in.data_ptr(), 2, d_in.data_ptr() + 100, 189, st)
    _refused(capi.EINVAL, "overlap", fr.work_device, d_out.data_ptr() + 2 * fr.kbch_bytes - 1, 2, d_out.data_ptr(), 189, st)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all()
    assert fr.counters(st) == before and fr.need(2, 189) == -(-5 * 189 // TS) - need
    got, _ = _run(fr, ups[need * TS:], 5, 189, in_off=3, out_off=1)  # the next good call continues the stream
    assert np.array_equal(got, want[3:8]) and got[0, 0] == 0xF2
    c = C.c_void_p()
    assert capi.lib.dvbs2_bbframer_counters(fr._h, None, None) == capi.EINVAL and b"out" in capi.lib.dvbs2_last_error()
    assert capi.lib.dvbs2_bbframer_need(fr._h, 1, 0, None) == capi.EINVAL and b"n_packets" in capi.lib.dvbs2_last_error()
    assert capi.lib.dvbs2_bbframer_create_raw(None, kbch, 8, 0) == capi.EINVAL and not c
    fr.close()
