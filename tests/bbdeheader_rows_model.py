"""The model of the de-header rows (include/dvbs2_fec_hip.h, "de-header rows"): one OracleBbDeheader per stream -- the plain-C restatement
of bbdeheader_bb, stateful like the block -- plus the offsets arithmetic. A stream that gets no frame in a call is not called at all."""
from math import ceil

import numpy as np

import fec_testlib as T
from dvbs2rx_amd import BBDEHEADER_STATE
from test_bbdeheader import _fuzz_stream

TS = 188


def healthy(kbch, n_frames, seed):
    """(user packets, n_frames BBFRAMEs that carry them back to back at the largest DFL)"""
    dflb = (kbch - 80) // 8
    ups = T.ts_up_stream(int(ceil(n_frames * dflb / TS)), np.random.default_rng(seed))
    return ups, T.bbframe_stream(kbch, n_frames, ups)


def fuzzed(kbch, n_frames, seed):
    """everything the block reacts to (tests/test_bbdeheader.py)"""
    return _fuzz_stream(kbch, n_frames, seed)


def bad_headers(kbch, n_frames, seed):
    """a healthy stream whose every header fails its CRC"""
    fr = healthy(kbch, n_frames, seed)[1]
    fr[:, 9] ^= 0xFF
    return fr


def pack(frames, kbch_bytes):
    """per-stream frame arrays [n_s, kbch_bytes] (n_s may be 0) -> (all frames stream-major [total, kbch_bytes], offsets int32 [S + 1])"""
    counts = [len(f) for f in frames]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    parts = [np.asarray(f, np.uint8).reshape(-1, kbch_bytes) for f in frames if len(f)]
    bb = np.concatenate(parts) if parts else np.zeros((0, kbch_bytes), np.uint8)
    return np.ascontiguousarray(bb), offsets


class Rows:
    def __init__(self, kbch_bits, n_streams):
        self.kbch_bits, self.kbch_bytes, self.S = kbch_bits, kbch_bits // 8, n_streams
        self.reset()

    def reset(self, stream=None):
        """all streams, or one: the block as constructed"""
        if stream is None:
            self.orc, self.last = [T.OracleBbDeheader(self.kbch_bits) for _ in range(self.S)], [0] * self.S
        else:
            self.orc[stream], self.last[stream] = T.OracleBbDeheader(self.kbch_bits), 0

    def call(self, frames):
        """frames[s]: the BBFRAMEs of stream s in this call -> (the TS bytes per stream, pkt_offsets as a list of S + 1)"""
        assert len(frames) == self.S
        out = []
        for s, f in enumerate(frames):
            if len(f) == 0:
                out.append(np.zeros(0, np.uint8))
                continue
            out.append(self.orc[s].work(f))
            self.last[s] = out[-1].size // TS
        return out, np.concatenate([[0], np.cumsum([o.size // TS for o in out])]).tolist()

    def counters(self):
        return [o.counters() for o in self.orc]

    def records(self):
        """the records a device call leaves behind, from all-zero records: partial_pkt holds the carried bytes and zeros behind them
        only as long as no LONGER partial was saved before -- compare through canon() where calls were cut"""
        r = np.zeros(self.S, BBDEHEADER_STATE)
        for s, o in enumerate(self.orc):
            c = o.counters()
            for k in ("synched", "partial_ts_bytes", "packets", "errors", "bbframes", "dropped", "gaps", "overruns"):
                r[s][k] = c[k]
            r[s]["last_packets"] = self.last[s]
            n = c["partial_ts_bytes"]
            r[s]["partial_pkt"][:n] = np.frombuffer(bytes(o.s.partial_pkt), np.uint8)[:n]
        return r


def canon(records, last_packets=True):
    """records with what does not count zeroed: the bytes of partial_pkt behind partial_ts_bytes (a shorter partial leaves the tail of a
    longer one in place, on the device as in the oracle) and, between runs cut differently, last_packets"""
    r = np.array(records, BBDEHEADER_STATE).reshape(-1).copy()
    for rec in r:
        rec["partial_pkt"][max(int(rec["partial_ts_bytes"]), 0):] = 0
        if not last_packets:
            rec["last_packets"] = 0
    return r
