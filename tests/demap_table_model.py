"""What the tests of the caller-table demapper (dvbs2_demap_create_table) need beyond tests/apsk_model.py, which is generic in the
table size: test constellations (rings with a seeded labelling, Gray QAM), the mapper and the LLR layout through column[], and the
inputs shared by the CPU and the GPU tests.

Conventions (include/dvbs2_fec_hip.h): entry i of a table is the point with label i; column[c] is the label bit (0 = the most
significant) whose LLRs fill column c of a frame: byte c * n_syms + j of a frame is the LLR of label bit column[c] of symbol j.
These tables are test material, not any standard's."""
import functools

import numpy as np

import apsk_model as A

N0_FRAMES = np.array([0.05, 0.01, 0.002], np.float32)  # at 0.2 a 256-point table yields only 6 or 7 distinct LLR values
# the N0 of the one-N0-for-all-frames call. The 64-point ring table takes 0.001, chosen with the float32 model so that a frame
# saturates in 5 .. 25 % of its LLRs (0.174 of frame 0; 0.037 at 0.002, 0.32 at 0.0007); the 8- and 4-point tables saturate nearly
# everywhere from N0 = 0.004 down, the 256-point one in 0.3 % at 0.002.
ONE_N0 = {"ring64": np.float32(0.001)}
SATURATION_CASE = "64ring-short-permuted"


def ring_table(sizes, radii, seed):
    """Ring k: sizes[k] points at radius radii[k] and angles 2 pi i / n, even rings (0, 2, ...) offset by pi / n; scaled to Es = 1;
    the labels are a seeded permutation (max-log over all points does not care about the labelling). complex128, entry i = label i."""
    pts = []
    for k, (n, r) in enumerate(zip(sizes, radii)):
        ang = 2.0 * np.pi * np.arange(n) / n + (np.pi / n if k % 2 == 0 else 0.0)
        pts.append(r * np.exp(1j * ang))
    p = np.concatenate(pts)
    assert len(p) & (len(p) - 1) == 0
    p = p / np.sqrt(np.mean(np.abs(p) ** 2))
    return p[np.random.default_rng(seed).permutation(len(p))]


RING8 = ring_table((1, 7), (0.0, 1.0), 8)  # a point at the origin
RING64 = ring_table((4, 12, 20, 28), (1.0, 2.2, 3.4, 4.6), 64)
RING256 = ring_table((32,) * 8, tuple(1.0 + 0.75 * k for k in range(8)), 256)
FOUR = ring_table((4,), (1.0,), 4)


def gray_qam(n_mod):
    """Square Gray QAM: h = n_mod / 2, axis levels 2 k - (2^h - 1), position k carries the Gray label k ^ (k >> 1); the upper h label
    bits select the real axis, the lower h the imaginary axis; Es = 1."""
    assert n_mod % 2 == 0
    h = n_mod // 2
    level = np.empty(1 << h)
    for k in range(1 << h):
        level[k ^ (k >> 1)] = 2 * k - ((1 << h) - 1)
    lab = np.arange(1 << n_mod)
    p = level[lab >> h] + 1j * level[lab & ((1 << h) - 1)]
    return p / np.sqrt(np.mean(np.abs(p) ** 2))


def natural(n_mod):
    return list(range(n_mod))


def map_bits_columns(cw_bits, pts, column):
    """The mapper through column[]: codeword bits (nf, N) -> symbols (nf, N / n_mod); bit c * rows + j of a frame is label bit
    column[c] of symbol j."""
    n_mod = int(np.log2(len(pts)))
    nf, N = cw_bits.shape
    rows = N // n_mod
    cols = cw_bits.reshape(nf, n_mod, rows).astype(np.int64)
    labels = np.zeros((nf, rows), np.int64)
    for c in range(n_mod):
        labels |= cols[:, c, :] << (n_mod - 1 - column[c])
    return np.asarray(pts)[labels]


def permute_columns(llr, n_mod, column):
    """Natural-order frames (nf, n_mod * rows) of apsk_model.demap_f32 (column b = label bit b) -> the column[] layout."""
    nf = llr.shape[0]
    return np.ascontiguousarray(llr.reshape(nf, n_mod, -1)[:, list(column), :]).reshape(nf, -1)


def unpermute_columns(llr, n_mod, column):
    """The inverse: a column[] layout back to the natural order (what apsk_model.check_vs_f64 and snr_f64 read)."""
    nf = llr.shape[0]
    out = np.empty((nf, n_mod, llr.shape[1] // n_mod), llr.dtype)
    out[:, list(column), :] = llr.reshape(nf, n_mod, -1)
    return out.reshape(nf, -1)


# ---- the demapper cases of tests/test_demap_table_gpu.py; test_demap_table_model.py checks the same inputs on the CPU
SHORT, NORMAL, MEDIUM = 0, 1, 2
N_LLR = {SHORT: 16200, NORMAL: 64800, MEDIUM: 32400}
TABLES = {"four": FOUR, "ring8": RING8, "ring64": RING64, "ring256": RING256}
# (id, table, framesize, column or None, what it reaches)
CASES = [("256ring-short", "ring256", SHORT, None),                           # n_syms 2025: odd columns on odd bytes, one symbol in the last quad
         ("256ring-medium-permuted", "ring256", MEDIUM, (7, 0, 6, 1, 5, 2, 4, 3)),  # 4050: odd columns 2 bytes off a dword
         ("64ring-short-permuted", "ring64", SHORT, (2, 1, 0, 5, 3, 4)),      # 2700: aligned columns
         ("64ring-normal", "ring64", NORMAL, None),                           # 10800
         ("8ring-short", "ring8", SHORT, None),                               # 5400: small table, ties at 0
         ("4-short", "four", SHORT, None)]                                    # 8100: the lower bound


def planted(rows):
    return [0, 1, rows - 2, rows - 1, 1000, 1001, 1002, 2001, 2002, 2003]


@functools.lru_cache(maxsize=None)
def demap_case(table, framesize):
    """3 frames of point + noise at N0 = N0_FRAMES, the symbols 0 and (1e3, -1e3) planted at both ends and inside (as
    test_apsk_gpu.demap_case); the float32 model's NATURAL-order LLRs for the per-frame N0 and for one N0 on all frames.
    Computed once, never modified. Returns (syms, per_frame, one, table complex128, table complex64, the one N0)."""
    p = TABLES[table]
    n_mod = int(np.log2(len(p)))
    rows = N_LLR[framesize] // n_mod
    rng = np.random.default_rng(rows + len(p))
    tx = p[rng.integers(0, len(p), (3, rows))]
    noise = np.sqrt(N0_FRAMES.astype(np.float64) / 2.0)[:, None] * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))
    syms = (tx + noise).astype(np.complex64)
    for f in range(3):
        syms[f, [0, rows - 2, 1000 + f]] = 0
        syms[f, [1, rows - 1, 2001 + f]] = 1e3 - 1e3j
    p32 = p.astype(np.complex64)
    per_frame = A.demap_f32(syms, N0_FRAMES, p32)[0]
    one_n0 = ONE_N0.get(table, N0_FRAMES[2])
    one = A.demap_f32(syms, one_n0, p32)[0]
    for a in (syms, per_frame, one, p32):
        a.setflags(write=False)
    return syms, per_frame, one, p, p32, one_n0


def unplanted(rows, n_mod):
    """(mask of the symbols that are not planted, their byte positions in a natural-order frame)"""
    keep = np.ones(rows, bool)
    keep[planted(rows)] = False
    return keep, np.concatenate([np.flatnonzero(keep) + c * rows for c in range(n_mod)])


# ---- the end-to-end operating points (short 3/4, S2_TABLE_C7): table, column, Es/N0 in dB
E2E = {"qam64": (6, (2, 1, 0, 5, 3, 4), 17.5), "qam256": (8, (7, 0, 6, 1, 5, 2, 4, 3), 22.5)}
E2E_FRAMES, E2E_GROUP, E2E_TRIALS, E2E_TABLE = 8, 8, 50, "S2_TABLE_C7"


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    """8 encoded short 3/4 frames through the mapper with column[] and AWGN. Returns (sent bytes, codeword bits, symbols, N0, table)."""
    import fec_testlib as T
    from dvbs2rx_amd import capi, get_fec_info
    n_mod, column, es_n0_db = E2E[name]
    fi = get_fec_info(capi.STANDARD_DVBS2, SHORT, "C3_4")
    assert fi["table"] == E2E_TABLE
    m, prim = T.BCH_FIELDS[SHORT]
    ob = T.OracleBch(m, prim, fi["bch_t"], fi["bch_n"])
    rng = np.random.default_rng(500 + n_mod)
    sent = rng.integers(0, 256, (E2E_FRAMES, fi["bch_k"] // 8), dtype=np.uint8)
    cw = T.ldpc_encode(fi["table"], np.unpackbits(ob.encode_bytes(sent), axis=1))
    p = gray_qam(n_mod)
    n0 = np.float32(10.0 ** (-es_n0_db / 10.0))
    tx = map_bits_columns(cw, p, column)
    syms = (tx + np.sqrt(float(n0) / 2.0) * (rng.normal(size=tx.shape) + 1j * rng.normal(size=tx.shape))).astype(np.complex64)
    for a in (sent, cw, syms):
        a.setflags(write=False)
    return sent, cw, syms, n0, p
