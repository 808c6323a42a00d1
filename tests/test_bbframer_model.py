"""CPU: the numpy model of BB framing (tests/bbframer_model.py) against what pins it -- the restatement of the reference's QA in
fec_testlib (bbframe_stream), the padded_dfl construction of tests/test_bbdeheader.py, the reference's genuine CRC where oracle/_ref
holds it, and the reference's receiver in its pinned restatement T.OracleBbDeheader. The GPU tests compare the device with this model."""
from math import ceil

import numpy as np
import pytest

import fec_testlib as T
from bbframer_model import TS, BbFramerModel, dfl_list, expected_packets

KBCHS = (3072, 7032, 14232, 16008, 58192)


def _ups(n, seed):
    return T.ts_up_stream(n, np.random.default_rng(seed))


def _one_call(kbch, n_frames, dfl, seed):
    m = BbFramerModel(kbch)
    ups = _ups(m.need(n_frames, dfl), seed)
    return ups, m.work(ups, n_frames, dfl), m


@pytest.mark.parametrize("kbch", KBCHS)
def test_largest_datafield_equals_bbframe_stream(kbch):
    """(a) dfl_bytes = 0 from pos = 0 is T.bbframe_stream byte for byte."""
    ups, frames, m = _one_call(kbch, 9, 0, 1)
    assert ups.size == TS * ceil(9 * (kbch // 8 - 10) / TS) and m.packets_read * TS == ups.size
    assert np.array_equal(frames, T.bbframe_stream(kbch, 9, ups))


def test_padded_dfl_construction():
    """(b) whole packets per frame: the padded_dfl case of tests/test_bbdeheader.py, built here as it is built there."""
    kbch, n_bb = 16008, 4
    per = ((kbch - 80) // 8) // TS
    dfl = per * TS
    ups = _ups(n_bb * per, 5)
    enc = T.ts_crc_encode(ups)
    want = np.zeros((n_bb, kbch // 8), np.uint8)
    for i in range(n_bb):
        want[i, :10] = T.bbheader(kbch, 0, dfl * 8)
        want[i, 10:10 + dfl] = enc[i * dfl:(i + 1) * dfl]
    m = BbFramerModel(kbch)
    assert m.need(n_bb, dfl) == n_bb * per
    assert np.array_equal(m.work(ups, n_bb, dfl), want)
    assert np.array_equal(T.OracleBbDeheader(kbch).work(want), ups[:-TS])


def test_crc_slots_against_the_reference_crc():
    """(c) every CRC slot of E makes the 188 bytes behind the packet's sync position divisible by the generator: with the restated
    remainder always, with the reference's own gf2_poly_rem where oracle/_ref holds it."""
    ref = T.ref_bch()
    ups, frames, m = _one_call(16008, 6, 0, 3)
    e = m.enc
    n = e.size // TS
    assert n > 60 and e[0] == 0x47
    for p in range(n - 1):
        piece = np.ascontiguousarray(e[p * TS + 1:(p + 1) * TS + 1])  # bytes 1..187 of packet p, then the slot of packet p + 1
        assert int(T.oracle().oracle_crc8_rem(T.ptr(piece), TS)) == 0
        assert e[(p + 1) * TS] == T.crc8_dvbs2(ups[p * TS + 1:(p + 1) * TS])
        if ref is not None:
            assert int(ref.ref_crc8_rem(T.ptr(piece), TS)) == 0


@pytest.mark.parametrize("kbch", (3072, 16008))
def test_call_split_is_invisible(kbch):
    """(d) a stream cut into random calls, empty ones among them, equals one call."""
    rng = np.random.default_rng(kbch)
    for dfl in dfl_list(kbch):
        ups, whole, m1 = _one_call(kbch, 40, dfl, 7)
        m = BbFramerModel(kbch)
        parts, f, pk = [], 0, 0
        while f < 40:
            n = min(int(rng.integers(0, 9)), 40 - f)
            need = m.need(n, dfl)
            parts.append(m.work(ups[pk * TS:(pk + need) * TS], n, dfl))
            assert m.packets_read == need and (n > 0 or need == 0)
            f += n
            pk += need
        assert pk * TS == ups.size and np.array_equal(np.concatenate(parts), whole)
        assert m.counters() == m1.counters() and m.pos == m1.pos == 40 * dfl


def _deheader_in_random_calls(kbch, frames, rng):
    orc = T.OracleBbDeheader(kbch)
    outs, i = [], 0
    while i < frames.shape[0]:
        n = int(rng.integers(0, 5))
        outs.append(orc.work(frames[i:i + n]))
        i += n
    return np.concatenate(outs), orc.counters()


@pytest.mark.parametrize("kbch", KBCHS)
def test_receiver_returns_the_packets(kbch):
    """(e) through the reference's receiver, calls cut at random: exactly packets 0 .. (total_bytes - 1) // 188 - 1, nothing counted."""
    rng = np.random.default_rng(kbch + 1)
    n_frames = 9
    for dfl in dfl_list(kbch):
        ups, frames, m = _one_call(kbch, n_frames, dfl, 11)
        got, c = _deheader_in_random_calls(kbch, frames, rng)
        n = expected_packets(n_frames * dfl)
        assert got.size == n * TS and np.array_equal(got, ups[:n * TS]), dfl
        assert c["errors"] == c["gaps"] == c["dropped"] == c["overruns"] == 0 and c["bbframes"] == n_frames and c["packets"] == n, dfl


def test_changing_dfl_comes_back_whole():
    """(f) dfl_bytes changes from call to call."""
    kbch = 16008
    rng = np.random.default_rng(17)
    dfls = dfl_list(kbch) + [0]
    m = BbFramerModel(kbch)
    ups = _ups(1200, 19)
    frames, pk, total = [], 0, 0
    for _ in range(30):
        n, dfl = int(rng.integers(0, 5)), int(rng.choice(dfls))
        need = m.need(n, dfl)
        frames.append(m.work(ups[pk * TS:(pk + need) * TS], n, dfl))
        pk += need
        total += n * (dfl or m.max_dfl_bytes)
    assert m.pos == total and pk == ceil(total / TS) and m.counters() == dict(packets=pk, bbframes=sum(f.shape[0] for f in frames), sync_errors=0)
    got, c = _deheader_in_random_calls(kbch, np.concatenate(frames), rng)
    n = expected_packets(total)
    assert n > 300 and got.size == n * TS and np.array_equal(got, ups[:n * TS])
    assert c["errors"] == c["gaps"] == c["dropped"] == c["overruns"] == 0


def test_wrong_sync_bytes_are_framed_and_counted():
    m = BbFramerModel(3072)
    ups = _ups(m.need(6), 23)
    ups[0] = 0x12
    ups[TS] = 0x34
    ups[-TS] = 0x56
    frames = m.work(ups, 6)
    assert m.counters() == dict(packets=ups.size // TS, bbframes=6, sync_errors=3)
    assert frames[0, 10] == 0x12 and m.enc[TS] == T.crc8_dvbs2(ups[1:TS])
