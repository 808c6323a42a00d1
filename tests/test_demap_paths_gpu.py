"""GPU: every path that turns symbols into LLRs -- the stand-alone demapper kernels, the demapper fused into the LDPC sweep
kernel's load under every kernel build, the APSK demapper launched in front of every build, the host entry's chunk loop -- and the
SNR estimators, against the CPU restatement (bit-exact) and against the float64 reference of the formulas (fec_testlib.demap_f64 /
snr_f64). Inputs: exact float32 ties, saturation edges, +-0, zeros, +-inf (QPSK), very small and very large N0, and one N0 per
frame."""
import functools
import json
import os

import numpy as np
import pytest

import apsk_model
import fec_testlib as T
from dvbs2rx_amd import Demapper, FecChain, apsk_points, capi, get_fec_info

pytestmark = pytest.mark.gpu

FS_NAME = {capi.FECFRAME_NORMAL: "normal", capi.FECFRAME_SHORT: "short", capi.FECFRAME_MEDIUM: "medium"}
CONST_SIZE = {capi.MOD_QPSK: 4, capi.MOD_8PSK: 8}  # what the checkers take
RATE_OF_ORDER = {0: "C3_4", 1: "C3_5", 2: "C25_36"}  # (the demapper uses the rate for its column order only)
# per-frame N0 of the edge frames: both ends of the float range (2 sqrt 2 / N0 and 4 / N0 still finite), and values at which the
# float32 search reaches the ties 126.5, 127.5, -127.5, -128.5, +-0.5, +-1.5 (test_demap_reference.TIE_N0)
EDGE_N0 = {4: (3e-30, 0.005, 0.3, 1.0, 1000.0, 3e30), 8: (1e-30, 0.001, 0.7, 1.0, 50.0, 3e30)}
CAP, G = 20, 32
APSK = (capi.MOD_16APSK, capi.MOD_32APSK)
APSK_NAME = {capi.MOD_16APSK: "16apsk", capi.MOD_32APSK: "32apsk"}
# Es/N0 [dB] of quasi-error-free operation, EN 302 307-1 table 13
APSK_QEF_DB = {(capi.MOD_16APSK, "C2_3"): 8.97, (capi.MOD_16APSK, "C3_4"): 10.21, (capi.MOD_16APSK, "C4_5"): 11.03,
               (capi.MOD_16APSK, "C5_6"): 11.61, (capi.MOD_16APSK, "C8_9"): 12.89, (capi.MOD_16APSK, "C9_10"): 13.13,
               (capi.MOD_32APSK, "C3_4"): 12.73, (capi.MOD_32APSK, "C4_5"): 13.64, (capi.MOD_32APSK, "C5_6"): 14.28,
               (capi.MOD_32APSK, "C8_9"): 15.69, (capi.MOD_32APSK, "C9_10"): 16.05}
APSK_MARGIN_DB = 3.0  # above table 13, as in test_apsk_gpu.py
# (constellation, rate, frame size) -> margin of a row whose CPU chain alone does not return every decodable frame at 3 dB and
# cap 20, raised in 0.5 dB steps until it does. Empty: the CPU chain returns all 29 decodable frames of all 20 rows at 3 dB.
APSK_ROW_MARGIN_DB = {}
APSK_EDGE_N0 = (0.2, 0.05, 0.01)  # the N0 of test_apsk_gpu.N0_FRAMES: what apsk_model.check_vs_f64 accepts for the restatement
APSK_ROWS = [(mod, rate, fs) for mod, rates in ((capi.MOD_16APSK, apsk_model.GAMMA_16), (capi.MOD_32APSK, apsk_model.GAMMA_32))
             for rate in rates for fs in ((capi.FECFRAME_NORMAL,) if rate == "C9_10" else (capi.FECFRAME_NORMAL, capi.FECFRAME_SHORT))]


def apsk_edge_frame(ns, n0, points_sent, k, rng):
    """One frame of point + noise at this N0 with the planted symbols of test_apsk_gpu.demap_case: 0 and (1e3, -1e3) at both ends
    and in the middle (k moves the middle ones from frame to frame)."""
    fr = (points_sent + np.sqrt(n0 / 2) * (rng.normal(size=ns) + 1j * rng.normal(size=ns))).astype(np.complex64)
    fr[[0, ns - 2, 1000 + k % 3]] = 0
    fr[[1, ns - 1, 2001 + k % 3]] = 1e3 - 1e3j
    return fr


def edge_frame(ns, n0, constellation, rng):
    """One frame: wide-range Gaussian symbols with every edge symbol of this N0 scattered over it several times (first and last
    positions included)."""
    scale = 10.0 ** rng.uniform(-4, 1, ns)
    fr = (scale * (rng.normal(size=ns) + 1j * rng.normal(size=ns))).astype(np.complex64)
    e = T.edge_symbols(n0, constellation)
    reps = min(8, ns // (2 * e.size))
    pos = rng.permutation(ns)[:reps * e.size]
    fr[pos] = np.tile(e, reps)
    fr[0], fr[-1] = e[0], e[-1]
    return fr


# ------------------------------------------------------------------ stand-alone demapper kernels
@pytest.mark.parametrize("framesize", [capi.FECFRAME_NORMAL, capi.FECFRAME_SHORT, capi.FECFRAME_MEDIUM], ids=FS_NAME.get)
@pytest.mark.parametrize("constellation,order", [(capi.MOD_QPSK, 0), (capi.MOD_8PSK, 0), (capi.MOD_8PSK, 1), (capi.MOD_8PSK, 2)],
                         ids=["qpsk", "8psk-012", "8psk-210", "8psk-102"])
def test_demap_kernels_edges(framesize, constellation, order):
    """Demapper.work on edge frames with one N0 per frame: bit-exact against the restatement, and against demap_f64 with the
    near-tie rule; the same with one N0 for all frames."""
    c = CONST_SIZE[constellation]
    dm = Demapper(framesize=framesize, rate=RATE_OF_ORDER[order], constellation=constellation, max_frames=len(EDGE_N0[c]))
    assert dm.column_order == order
    rng = np.random.default_rng(framesize * 10 + c + order)
    n0 = np.array(EDGE_N0[c], np.float32)
    syms = np.stack([edge_frame(dm.n_syms, float(v), c, rng) for v in n0])
    got = dm.work(syms, n0)
    assert np.array_equal(got, T.oracle_demap(syms, n0, c, order))
    near = T.check_demap_vs_f64(got, syms, n0, c, order, "per-frame N0")
    print(f"{FS_NAME[framesize]} constellation {c} order {order}: {near} near-tie LLRs of {got.size}")
    one = dm.work(syms[::-1], n0[2])
    assert np.array_equal(one, T.oracle_demap(syms[::-1], n0[2], c, order))
    T.check_demap_vs_f64(one, syms[::-1], n0[2], c, order, "one N0")
    dm.close()


def test_demap_exact_ties_on_gpu():
    """A frame made only of exact ties (and saturation points) per constellation: the kernels round them to even."""
    for constellation in (capi.MOD_QPSK, capi.MOD_8PSK):
        c = CONST_SIZE[constellation]
        dm = Demapper(framesize=capi.FECFRAME_SHORT, rate="C1_2", constellation=constellation, max_frames=4)
        n0 = np.array([0.3, 1000.0, 3e30, 0.005] if c == 4 else [0.7, 0.001, 50.0, 3e30], np.float32)
        syms = np.zeros((4, dm.n_syms), np.complex64)
        for f, v in enumerate(n0):
            ties = np.array(list(T.tie_symbols(float(v), c).values()), np.complex64)
            syms[f] = np.resize(ties, dm.n_syms)
        got = dm.work(syms, n0)
        assert np.array_equal(got, T.oracle_demap(syms, n0, c, 0))
        for f, v in enumerate(n0):
            pre = T.demap_f32_pre(syms[f], v, c)
            pre = pre if c == 4 else np.concatenate(pre)  # order 0: b0, b1, b2 columns
            assert np.array_equal(got[f], T.quantise_f64(pre.astype(np.float64)))
            assert (np.abs(pre - np.trunc(pre)) == 0.5).sum() >= dm.n_syms // 2  # at least one exact tie per symbol on average
        dm.close()


@pytest.mark.parametrize("framesize", [capi.FECFRAME_NORMAL, capi.FECFRAME_SHORT], ids=FS_NAME.get)
def test_column_order_every_rate(framesize):
    """Demapper.column_order for every rate of that frame size against the reference's rule by rate name."""
    rows = json.load(open(os.path.join(T.ROOT, "tests", "golden", "fec_params.json")))["rows"]
    names = sorted({r["rate"] for r in rows if r["framesize_id"] == framesize})
    for name in names:
        dm = Demapper(framesize=framesize, rate=name, constellation=capi.MOD_8PSK, max_frames=1)
        assert dm.column_order == T.column_order(name), name
        dm.close()


def test_host_wrappers_convert_symbol_dtypes():
    """complex128 / float64 symbols are converted, not reinterpreted as float32 pairs; other dtypes are refused."""
    dm = Demapper(framesize=capi.FECFRAME_SHORT, rate="C3_5", constellation=capi.MOD_8PSK, max_frames=2)
    rng = np.random.default_rng(4)
    syms = (rng.normal(size=(2, dm.n_syms)) + 1j * rng.normal(size=(2, dm.n_syms))).astype(np.complex64)
    want = dm.work(syms, 0.5)
    assert np.array_equal(dm.work(syms.astype(np.complex128), 0.5), want)
    with pytest.raises(TypeError):
        dm.work(syms.real, 0.5)
    dm.close()
    chain = FecChain(framesize=capi.FECFRAME_SHORT, rate="C1_2", constellation=capi.MOD_QPSK, max_frames=2, max_trials=5)
    syms = (rng.normal(size=(2, chain.n_syms)) + 1j * rng.normal(size=(2, chain.n_syms))).astype(np.complex64)
    want = chain.work(syms, 0.5)
    for form in (syms.astype(np.complex128), syms.view(np.float32).astype(np.float64)):
        got = chain.work(form, 0.5)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(TypeError):
        chain.work(syms.view(np.float32).astype(np.int32), 0.5)
    with pytest.raises(ValueError):
        chain.work(syms[:, :-1], 0.5)
    chain.close()


# ------------------------------------------------------------------ SNR estimators
def snr_rtol_gpu(n):
    """demap_snr_kernel: 256 threads each sum ceil(n / 256) <= 127 terms in order, then an 8-level tree: <= ceil(n / 256) + 8
    additions of positive terms, each term carrying <= 4 u (x - s, two squares, their sum) -> (ceil(n / 256) + 11) u on each sum,
    one u for the quotient. 32400 symbols: 277 u = 1.65e-5."""
    return (2 * (-(-n // 256) + 11) + 1) * T.U32


def snr_frames(ns, c, order, rng):
    """Frames of reference points (float constants) from random bits, the matching decoded LLRs (0 for some '0' bits, -128 for
    some '1' bits), plus noise of a few powers; the last two frames noiseless and all-zero. Large-error symbols at 0, 255, 256,
    n - 256, n - 1, each a distinct 1-3 % of its frame's noise: a skipped or double-counted one moves the estimate by >> rtol."""
    nf = 5
    bits = rng.integers(0, 2, (nf, ns * (2 if c == 4 else 3))).astype(np.uint8)
    llr = np.where(bits == 1, rng.integers(-128, 0, bits.shape), rng.integers(0, 128, bits.shape)).astype(np.int8)
    llr[:, 1::7] = np.where(bits[:, 1::7] == 1, -128, 0)
    if c == 4:
        pts = (np.where(bits[:, 0::2], -T.RS2_F32, T.RS2_F32) + 1j * np.where(bits[:, 1::2], -T.RS2_F32, T.RS2_F32)).astype(np.complex64)
    else:
        ra = T.column_bases(ns, order)
        pts = T.map_8psk(np.stack([bits[:, a:a + ns] for a in ra], axis=-1))
    sigma = np.array([0.03, 0.15, 0.5, 0, 0])[:, None]
    syms = (pts + sigma * (rng.normal(size=pts.shape) + 1j * rng.normal(size=pts.shape))).astype(np.complex64)
    syms[4] = 0
    plant = [0, 255, 256, ns - 256, ns - 1]
    for f in range(3):
        total = np.sum(np.abs(syms[f].astype(np.complex128) - pts[f]) ** 2)
        for k, j in enumerate(plant):
            a = np.sqrt((0.01 + 0.005 * k) * total)  # radial: the hard decision stays the sent point
            syms[f, j] = (pts[f, j] * (1 + a)).astype(np.complex64)
    return syms, llr, pts, plant


@pytest.mark.parametrize("framesize", [capi.FECFRAME_NORMAL, capi.FECFRAME_SHORT], ids=FS_NAME.get)
@pytest.mark.parametrize("constellation,order", [(capi.MOD_QPSK, 0), (capi.MOD_8PSK, 0), (capi.MOD_8PSK, 1), (capi.MOD_8PSK, 2)],
                         ids=["qpsk", "8psk-012", "8psk-210", "8psk-102"])
def test_snr_estimators_vs_float64(framesize, constellation, order):
    """estimate_snr (hard slice) and refine_snr (signs of decoded LLRs) against snr_f64 with the kernel's derived rtol; noiseless
    frames give the 1e-12 floor, all-zero frames ~1."""
    c = CONST_SIZE[constellation]
    dm = Demapper(framesize=framesize, rate=RATE_OF_ORDER[order], constellation=constellation, max_frames=5)
    rng = np.random.default_rng(50 + c + order + framesize)
    syms, llr, pts, plant = snr_frames(dm.n_syms, c, order, rng)
    rtol = snr_rtol_gpu(dm.n_syms)
    for f in range(3):  # the planted symbols are visible: leaving out any one changes the estimate by > 100 rtol
        full = T.snr_f64(syms[f:f + 1], c, llr[f:f + 1], order)[0]
        for j in plant:
            keep = np.ones(dm.n_syms, bool); keep[j] = False
            x, p = syms[f][keep].astype(np.complex128), pts[f][keep]
            assert abs(np.sum(np.abs(p) ** 2) / np.sum(np.abs(x - p) ** 2) / full - 1) > 100 * rtol
    got, want = dm.estimate_snr(syms).astype(np.float64), T.snr_f64(syms, c)
    assert np.allclose(got, want, rtol=rtol, atol=0), (got, want, rtol)
    assert want[3] > 1e15 and abs(want[4] - 1) < 1e-6
    got, want = dm.refine_snr(syms, llr).astype(np.float64), T.snr_f64(syms, c, llr, order)
    assert np.allclose(got, want, rtol=rtol, atol=0), (got, want, rtol)
    dm.close()


# ------------------------------------------------------------------ chains: fused load / demapper launch, every MODCOD
def _modcods():
    rows = json.load(open(os.path.join(T.ROOT, "tests", "golden", "fec_params.json")))["rows"]
    seen = {}
    for r in rows:
        if r["framesize"] == "FECFRAME_MEDIUM":
            continue
        for mod in (capi.MOD_QPSK, capi.MOD_8PSK):
            order = T.column_order(r["rate"]) if mod == capi.MOD_8PSK else 0
            seen.setdefault((mod, r["table"], r["bch_n"], r["bch_t"], r["framesize_id"], order), r)
    return [pytest.param(r, mod, order, id=f"{'qpsk' if mod == capi.MOD_QPSK else '8psk'}-{r['standard'][-5:]}-{r['rate']}-"
                         f"{FS_NAME[r['framesize_id']]}") for (mod, _, _, _, _, order), r in seen.items()]


MODCODS = _modcods()


def threshold_db(rate, c):
    """Es/N0 [dB] a little above where a code of this rate works on this constellation (capacity-like guide + margin)."""
    bps = 2 if c == 4 else 3
    return 10 * np.log10(2 ** (bps * rate) - 1) + (5.0 if c == 4 else 6.0)  # (cap 20: low-rate codes need the margin)


@functools.lru_cache(maxsize=4)  # (the sweep-kernel builds reuse one case)
def chain_case(standard, framesize, rate, constellation, nf, seed):
    """nf frames for one MODCOD with one N0 per frame: decodable frames (Es/N0 0-1.5 dB above threshold_db; 16APSK / 32APSK: above
    table 13 of EN 302 307-1 + the row's margin), noise-only frames and edge/tie frames (APSK: apsk_edge_frame) in every whole group
    of 32, decodable frames only in the tail (its CPU decode uses the scalar restatement).
    Returns (symbols, per-frame N0, sent messages, decodable mask, CPU chain for per-frame N0, CPU chain for N0 = n0[0])."""
    apsk = constellation in APSK
    c = 2 ** apsk_model.N_MOD[constellation] if apsk else CONST_SIZE[constellation]
    fi = get_fec_info(standard, framesize, rate)
    m, prim = T.BCH_FIELDS[framesize]
    ob = T.OracleBch(m, prim, fi["bch_t"], fi["bch_n"])
    rng = np.random.default_rng(seed)
    sent = rng.integers(0, 256, (nf, fi["bch_k"] // 8), dtype=np.uint8)
    info = np.zeros((nf, T.ldpc_info(fi["table"])[1]), np.uint8)  # shortened codes (VLSNR): the bits past the BCH codeword are 0
    info[:, :fi["bch_n"]] = np.unpackbits(ob.encode_bytes(sent), axis=1)
    cw = T.ldpc_encode(fi["table"], info)
    if apsk:
        pts = apsk_model.map_bits(cw, apsk_model.points(constellation, rate))  # natural column order
    elif c == 4:
        pts = ((1 - 2.0 * cw[:, 0::2]) + 1j * (1 - 2.0 * cw[:, 1::2])) * np.sqrt(0.5)
    else:
        rows = cw.shape[1] // 3
        pts = T.map_8psk(np.stack([cw[:, a:a + rows] for a in T.column_bases(rows, T.column_order(rate))], axis=-1))
    ns = pts.shape[1]
    if apsk:
        base_db = APSK_QEF_DB[constellation, rate] + APSK_ROW_MARGIN_DB.get((constellation, rate, framesize), APSK_MARGIN_DB)
    else:
        base_db = threshold_db(fi["ldpc_k"] / fi["ldpc_n"], c)
    es_n0 = base_db + rng.uniform(0, 1.5, nf)
    n0 = (10 ** (-es_n0 / 10)).astype(np.float32)
    kind = np.zeros(nf, int)  # 0 decodable, 1 noise, 2 edge / ties; in every whole group of 32
    whole = np.arange(nf - nf % G)
    kind[whole[np.isin(whole % G, (3, 12, 25))]] = 1
    kind[whole[np.isin(whole % G, (7, 18, 30))]] = 2
    syms = np.empty((nf, ns), np.complex64)
    for f in range(nf):
        if kind[f] == 2 and apsk:
            k = int((kind[:f] == 2).sum())  # the N0 cycles over the edge frames
            n0[f] = APSK_EDGE_N0[k % 3]
            syms[f] = apsk_edge_frame(ns, float(n0[f]), pts[f], k, rng)
            continue
        if kind[f] == 2:
            n0[f] = EDGE_N0[c][1 + f % 4]
            syms[f] = edge_frame(ns, float(n0[f]), c, rng)
            continue
        noise = np.sqrt(n0[f] / 2) * (rng.normal(size=ns) + 1j * rng.normal(size=ns))
        syms[f] = (noise * (3 / np.sqrt(n0[f])) if kind[f] == 1 else pts[f] + noise).astype(np.complex64)
    order = T.column_order(rate) if c == 8 else 0

    def cpu(n0_used):
        if apsk:  # the float32 restatement test_apsk_gpu.py holds the kernel to, on the library's float table
            llr = apsk_model.demap_f32(syms, n0_used, apsk_points(constellation, rate))[0]
        else:
            llr = T.oracle_demap(syms, n0_used, c, order)
        dec, ret = T.cpu_ldpc_decode_ragged(fi["table"], llr, G, CAP)
        msg, corr = ob.decode_bytes(T.pack_bits(dec, fi["bch_n"]))
        return msg, corr, ret

    return syms, n0, sent, kind == 0, cpu(n0), cpu(n0[0])


def run_modcod(standard, framesize, rate, constellation, nf=35, seed=1):
    """Both calls (one N0 per frame through the device entry, one N0 through the host entry) against the CPU chain. Returns the
    kernel the chain runs."""
    import torch
    syms, n0, sent, good, (wmsg, wcorr, wret), (wmsg1, wcorr1, wret1) = chain_case(standard, framesize, rate, constellation, nf, seed)
    assert (wcorr[good] >= 0).all() and np.array_equal(wmsg[good], sent[good])  # the comparison is not vacuous
    chain = FecChain(standard=standard, framesize=framesize, rate=rate, constellation=constellation, group_size=G, max_frames=nf,
                     max_trials=CAP)
    kname = chain.kernel_name
    d_syms = torch.from_numpy(syms.view(np.float32)).cuda()
    d_n0 = torch.from_numpy(n0).cuda()
    d_msg = torch.empty((nf, chain.msg_bytes), dtype=torch.uint8, device="cuda")
    d_ret = torch.empty(-(-nf // G), dtype=torch.int32, device="cuda")
    d_corr = torch.empty(nf, dtype=torch.int32, device="cuda")
    chain.work_device(d_syms.data_ptr(), nf, d_n0.data_ptr(), nf, d_msg.data_ptr(), d_ret.data_ptr(), d_corr.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_ret.cpu().tolist() == list(wret), kname
    assert d_corr.cpu().numpy().tolist() == wcorr.tolist(), kname
    bad = np.nonzero((d_msg.cpu().numpy() != wmsg).any(axis=1))[0]
    assert bad.size == 0, f"{kname}: frames {bad.tolist()} differ (per-frame N0)"
    msg, ret, corr = chain.work(syms, n0[0])
    assert ret.tolist() == list(wret1) and corr.tolist() == wcorr1.tolist(), kname
    assert np.array_equal(msg, wmsg1), f"{kname}: one N0"
    chain.close()
    return kname


def _std(r):
    return capi.STANDARD_DVBS2 if r["standard"] == "STANDARD_DVBS2" else capi.STANDARD_DVBT2


@pytest.mark.parametrize("row,constellation,order", MODCODS)
def test_chain_every_modcod(row, constellation, order, record_property):
    """Every (table, BCH code, frame size, column order) of fec_params.json with normal or short frames, QPSK and 8PSK: 35 frames
    (odd count, a tail group of 3, an idle half in the last pair workgroup) -> messages, BCH corrections and LDPC returns equal to
    the CPU chain. The kernel name tells whether the demapper ran fused into the sweep load or as its own launch."""
    kname = run_modcod(_std(row), row["framesize_id"], row["rate"], constellation)
    path = "demapper launch" if "_pr_" in kname else "fused load"
    record_property("demap_path", f"{path}: {kname}")
    print(f"\n{row['rate']} {FS_NAME[row['framesize_id']]} {'QPSK' if constellation == capi.MOD_QPSK else '8PSK'} order {order}: {path} ({kname})")


@pytest.mark.parametrize("constellation,rate,framesize", APSK_ROWS, ids=[f"{APSK_NAME[m]}-{r}-{FS_NAME[f]}" for m, r, f in APSK_ROWS])
def test_chain_every_apsk_modcod(constellation, rate, framesize, record_property):
    """Every legal (constellation, rate, frame size) of MODCODs 18-28, the same 35 frames as above: the chain runs the demapper as
    its own launch into the LLR buffer, then the sweep kernel and BCH from the LDPC state -> messages, BCH corrections and LDPC
    returns equal to the CPU chain (apsk_model.demap_f32 -> cpu_ldpc_decode_ragged -> OracleBch)."""
    good = chain_case(capi.STANDARD_DVBS2, framesize, rate, constellation, 35, 1)[3]
    assert good.sum() >= 26
    kname = run_modcod(capi.STANDARD_DVBS2, framesize, rate, constellation)
    record_property("demap_path", f"demapper launch: {kname}")
    print(f"\n{rate} {FS_NAME[framesize]} {APSK_NAME[constellation]}: demapper launch ({kname})")
    if framesize == capi.FECFRAME_NORMAL:
        assert "_pr_" not in kname  # demapper launch + classic kernel


def test_chain_medium_frames_refused():
    """Medium frames: the BCH stage cannot take them (k not a multiple of 8, as in the reference), so the chain is refused."""
    rows = json.load(open(os.path.join(T.ROOT, "tests", "golden", "fec_params.json")))["rows"]
    medium = [r for r in rows if r["framesize"] == "FECFRAME_MEDIUM"]
    assert medium
    for r in medium:
        for mod in (capi.MOD_QPSK, capi.MOD_8PSK):
            with pytest.raises(capi.Dvbs2Error) as e:
                FecChain(standard=_std(r), framesize=capi.FECFRAME_MEDIUM, rate=r["rate"], constellation=mod, max_frames=4)
            assert e.value.code == capi.EINVAL, r["rate"]


# ------------------------------------------------------------------ every sweep-kernel build on the fused path
FUSED_CONFIGS = [
    ("qpsk-1_2-normal", capi.FECFRAME_NORMAL, "C1_2", capi.MOD_QPSK),
    ("qpsk-1_3-normal", capi.FECFRAME_NORMAL, "C1_3", capi.MOD_QPSK),
    ("8psk-3_5-normal-210", capi.FECFRAME_NORMAL, "C3_5", capi.MOD_8PSK),
    ("8psk-25_36-normal-102", capi.FECFRAME_NORMAL, "C25_36", capi.MOD_8PSK),
    ("8psk-9_10-normal", capi.FECFRAME_NORMAL, "C9_10", capi.MOD_8PSK),    # degree class 32
    ("qpsk-8_9-short", capi.FECFRAME_SHORT, "C8_9", capi.MOD_QPSK),        # <28, hz2>
    ("8psk-3_5-short-210", capi.FECFRAME_SHORT, "C3_5", capi.MOD_8PSK),    # dense build
]


@pytest.mark.parametrize("variant", list(T.VARIANTS))
@pytest.mark.parametrize("name,framesize,rate,constellation", FUSED_CONFIGS, ids=[c[0] for c in FUSED_CONFIGS])
def test_fused_demap_every_build(name, framesize, rate, constellation, variant, monkeypatch):
    """Each sweep-kernel build with the demapper in its load gives the CPU chain's bytes; where a build forces the parity-in-records
    kernel the chain runs the stand-alone demapper, which must give the same bytes."""
    for k, v in T.VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    kname = run_modcod(capi.STANDARD_DVBS2, framesize, rate, constellation, nf=35, seed=7)
    print(f"\n{name} {variant}: {'demapper launch' if '_pr_' in kname else 'fused load'} ({kname})")


# ------------------------------------------------------------------ every sweep-kernel build behind the demapper launch
UNFUSED_CONFIGS = [
    ("16apsk-2_3-normal", capi.FECFRAME_NORMAL, "C2_3", capi.MOD_16APSK),
    ("32apsk-9_10-normal", capi.FECFRAME_NORMAL, "C9_10", capi.MOD_32APSK),  # degree class 32
    ("16apsk-8_9-short", capi.FECFRAME_SHORT, "C8_9", capi.MOD_16APSK),      # <28, hz2>
    ("32apsk-3_4-short", capi.FECFRAME_SHORT, "C3_4", capi.MOD_32APSK),
]


@pytest.mark.parametrize("variant", list(T.VARIANTS))
@pytest.mark.parametrize("name,framesize,rate,constellation", UNFUSED_CONFIGS, ids=[c[0] for c in UNFUSED_CONFIGS])
def test_unfused_demap_every_build(name, framesize, rate, constellation, variant, monkeypatch):
    """Each sweep-kernel build behind the stand-alone APSK demapper (LLR buffer -> int8 load -> BCH from the LDPC state) gives the
    CPU chain's bytes."""
    for k, v in T.VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    kname = run_modcod(capi.STANDARD_DVBS2, framesize, rate, constellation, nf=35, seed=7)
    print(f"\n{name} {variant}: demapper launch ({kname})")


# ------------------------------------------------------------------ host entry, chunked, one N0 per frame
@pytest.mark.parametrize("framesize,rate,constellation", [(capi.FECFRAME_NORMAL, "C1_2", capi.MOD_QPSK), (capi.FECFRAME_SHORT, "C1_4", capi.MOD_QPSK),
                                                          (capi.FECFRAME_SHORT, "C3_4", capi.MOD_16APSK)],
                         ids=["qpsk-1_2-normal-fused", "qpsk-1_4-short-pr", "16apsk-3_4-short-unfused"])
def test_host_entry_chunks_per_frame_n0(framesize, rate, constellation, monkeypatch):
    """dvbs2_chain_decode in chunks of 32 (six chunks) with a distinct N0 per frame, pageable and page-locked buffers: each chunk
    must hand its own frames' N0 to the demapper (fused load or launch; 16APSK: the launch writes the chunk's place in the LLR
    buffer and the LDPC stage starts at that frame)."""
    import torch
    monkeypatch.setenv("DVBS2_HOST_CHUNK", "32")
    nf = 163
    syms, n0, sent, good, (wmsg, wcorr, wret), _ = chain_case(capi.STANDARD_DVBS2, framesize, rate, constellation, nf, 11)
    assert (wcorr[good] >= 0).all() and np.array_equal(wmsg[good], sent[good])
    assert len(set(n0.tolist())) > nf * 3 // 4
    chain = FecChain(framesize=framesize, rate=rate, constellation=constellation, group_size=G, max_frames=nf, max_trials=CAP)
    print(f"\n{rate} {FS_NAME[framesize]}: {chain.kernel_name}")
    if constellation == capi.MOD_QPSK:
        assert ("_pr_" in chain.kernel_name) == (framesize == capi.FECFRAME_SHORT)
    msg, ret, corr = chain.work(syms, n0)
    assert ret.tolist() == list(wret) and corr.tolist() == wcorr.tolist()
    assert np.array_equal(msg, wmsg)
    hin = torch.from_numpy(syms.view(np.float32)).pin_memory()
    hn0 = torch.from_numpy(n0).pin_memory()
    hmsg = torch.zeros((nf, chain.msg_bytes), dtype=torch.uint8).pin_memory()
    hret = torch.zeros(-(-nf // G), dtype=torch.int32).pin_memory()
    hcorr = torch.zeros(nf, dtype=torch.int32).pin_memory()
    chain.work_host_ptr(hin.data_ptr(), nf, hn0.data_ptr(), nf, hmsg.data_ptr(), hret.data_ptr(), hcorr.data_ptr())
    assert hret.numpy().tolist() == list(wret) and hcorr.numpy().tolist() == wcorr.tolist()
    assert np.array_equal(hmsg.numpy(), wmsg)
    chain.close()
