"""A stateful numpy restatement of BB framing for MPEG-TS (EN 302 307-1 clauses 5.1.4 to 5.1.6) as dvbs2_bbframer_* defines it
(notes/bbframer.md, include/dvbs2_fec_hip.h): the CRC-encoded stream E over the packets presented so far, a position pos in it, and per
call (n_frames, dfl_bytes) BBFRAMEs of BBHEADER + E[s .. s + dfl_bytes) + zero padding. Built on the restatements of the reference's
own QA that fec_testlib already holds (crc8_dvbs2, bbheader)."""
import numpy as np

import fec_testlib as T

TS = 188
_TAB = np.array([T.crc8_dvbs2(bytes([r])) for r in range(256)], np.uint8)  # r * x^8 mod g: the check byte of the one-byte string r


def packet_crcs(packets):
    """T.crc8_dvbs2 of bytes 1..187 of every packet of an (n, 188) array, all packets at once."""
    reg = np.zeros(packets.shape[0], np.uint8)
    for i in range(1, TS):
        reg = _TAB[reg] ^ packets[:, i]
    return _TAB[reg]


class BbFramerModel:
    def __init__(self, kbch_bits):
        assert kbch_bits % 8 == 0
        self.kbch_bits = kbch_bits
        self.kbch_bytes = kbch_bits // 8
        self.max_dfl_bytes = self.kbch_bytes - 10
        self.matype = (0xF2, 0)
        self.reset()

    def reset(self):
        self.pos = 0
        self.enc = np.zeros(0, np.uint8)  # E over every packet presented since the reset
        self.prev_crc = None              # the CRC of the last packet presented
        self.packets = self.bbframes = self.sync_errors = 0

    def set_matype(self, matype1, matype2):
        self.matype = (matype1, matype2)

    def _dfl(self, dfl_bytes):
        dfl = dfl_bytes if dfl_bytes else self.max_dfl_bytes
        assert TS <= dfl <= self.max_dfl_bytes
        return dfl

    def need(self, n_frames, dfl_bytes=0):
        """Whole packets the next call reads: ceil((pos + n_frames * dfl) / 188) - ceil(pos / 188)."""
        end = self.pos + n_frames * self._dfl(dfl_bytes)
        return -(-end // TS) - -(-self.pos // TS)

    def _present(self, packets):
        p = np.array(packets, np.uint8).reshape(-1, TS)
        e = p.copy()
        if p.shape[0]:
            crc = packet_crcs(p)
            e[1:, 0] = crc[:-1]
            if self.prev_crc is not None:
                e[0, 0] = self.prev_crc  # (the very first packet keeps its own byte 0)
            self.prev_crc = int(crc[-1])
        self.sync_errors += int((p[:, 0] != 0x47).sum())
        self.packets += p.shape[0]
        self.enc = np.concatenate([self.enc, e.reshape(-1)])

    def work(self, ts, n_frames, dfl_bytes=0):
        """ts: at least need() packets, of which exactly need() are read (self.packets_read) -> (n_frames, kbch_bytes) uint8."""
        dfl = self._dfl(dfl_bytes)
        n = self.need(n_frames, dfl_bytes)
        self.packets_read = n
        out = np.zeros((n_frames, self.kbch_bytes), np.uint8)
        if n_frames == 0:
            return out
        self._present(np.asarray(ts, np.uint8).reshape(-1)[:n * TS])
        for f in range(n_frames):
            s = self.pos + f * dfl
            syncd = 8 * ((TS - s % TS) % TS)
            out[f, :10] = T.bbheader(self.kbch_bits, syncd, 8 * dfl, matype1=self.matype[0], matype2=self.matype[1])
            out[f, 10:10 + dfl] = self.enc[s:s + dfl]
        self.pos += n_frames * dfl
        self.bbframes += n_frames
        return out

    def counters(self):
        return dict(packets=self.packets, bbframes=self.bbframes, sync_errors=self.sync_errors)


def dfl_list(kbch_bits):
    """The DATAFIELD lengths the tests walk: the largest, whole packets per frame, an odd one, one packet, one packet and a byte, and
    375 (two packets less a byte) where it fits."""
    mx = kbch_bits // 8 - 10
    out = [mx, mx // TS * TS, mx - 5, 188, 189]
    if mx >= 375:
        out.append(375)
    return [d for d in dict.fromkeys(out) if TS <= d <= mx]


def expected_packets(total_bytes):
    """Packets the receiver returns from a stream of total_bytes DATAFIELD bytes that starts at pos = 0: a packet is released once the
    CRC in the next packet's sync position has arrived."""
    return max((total_bytes - 1) // TS, 0)
