"""PLFRAME front end on the device (dvbs2_plframe_*) against the float64 model of tests/plframe_model.py: hard PLSC modes bit
for bit, the soft mode, the phases and the fine frequency offset under bounds derived from the float32 format (every bound is
computed per value by the model), the payload step bit for bit against dvbs2_plpayload_process_device, and end to end into
the FEC chain. The estimates are UNPINNED against the genuine reference (VOLK and GNU Radio's fast_atan2f are not part of the
reference tree); the hard PLSC modes are exact."""
import ctypes as C

import numpy as np
import pytest

import fec_testlib as T
import plframe_model as M
from dvbs2rx_amd import FecChain, PlFrontEnd, PlPayload, capi, get_fec_info

pytestmark = pytest.mark.gpu

DUMMY = 0  # PLSC of the dummy frame: 36 slots, the smallest geometry -- PLSC decoding reads the header only


def plsc_of(modcod, short, pilots):
    return (modcod << 2) | (short << 1) | pilots


# (modcod, short) giving n_slots 360 / 240 / 180 / 144 / 90 / 36, each with and without pilots (the dummy frame has none
# whatever bit 0 says), gold codes and batch sizes going round
_G = [(4, 0), (13, 0), (18, 0), (24, 0), (4, 1), (0, 0), (13, 1)]
GEOMS = [(plsc_of(mc, sh, p), (0, 5, 131071)[i % 3], (3, 33, 1)[(i + p) % 3])
         for i, (mc, sh) in enumerate(_G) for p in (0, 1)]


def test_geometries_cover_the_slot_counts():
    assert {M.pls_parse(p)["n_slots"] for p, _, _ in GEOMS} >= {360, 240, 180, 144, 90, 36}
    assert {g for _, g, _ in GEOMS} == {0, 5, 131071} and {n for _, _, n in GEOMS} == {1, 3, 33}
    assert {bool(M.pls_parse(p)["n_pilots"]) for p, _, _ in GEOMS} == {True, False}


def run_device(fe, frames, cc, cf=None, trailing=None, payload=True, stream=None, want=None):
    """The _device entries on torch buffers; returns (xfecframes or None, dict of estimates) as numpy."""
    import torch
    nf = frames.shape[0]
    x = frames.reshape(-1) if trailing is None else np.concatenate([frames.reshape(-1), trailing])
    d_x = torch.from_numpy(np.ascontiguousarray(x).view(np.float32)).cuda()
    d_cc = torch.from_numpy(np.ascontiguousarray(cc, np.int32)).cuda()
    d_cf = torch.from_numpy(np.ascontiguousarray(cf, np.float32)).cuda() if cf is not None else None
    d_est = {k: torch.zeros((nf, fe.n_pilots) if k == "pilot_phase" else (nf,), dtype=getattr(torch, np.dtype(dt).name), device="cuda")
             for k, dt in PlFrontEnd.EST if want is None or k in want}
    d_out = torch.zeros((nf, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda") if payload else None
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        fe.work_device(d_x.data_ptr(), nf, trailing is not None, d_cc.data_ptr(), d_cf.data_ptr() if d_cf is not None else 0,
                       d_out.data_ptr() if payload else 0, st.cuda_stream,
                       **{k: (v.data_ptr() if v.numel() else 0) for k, v in d_est.items()})
    st.synchronize()
    out = d_out.cpu().numpy().view(np.complex64) if payload else None
    return out, {k: v.cpu().numpy() for k, v in d_est.items()}


def headers_to_frames(headers, rng):
    """whole dummy-geometry PLFRAMEs around the given (n, 90) headers"""
    n = headers.shape[0]
    L = M.pls_parse(DUMMY)["plframe_len"]
    x = (rng.normal(size=(n, L)) + 1j * rng.normal(size=(n, L))) * M.S
    x[:, :90] = headers
    return x.astype(np.complex64)


def decode_on_device(headers, rng, coherent, soft, enabled=None):
    fe = PlFrontEnd(0, DUMMY, max_frames=headers.shape[0], coherent=coherent, soft=soft, expected_pls=enabled)
    frames = headers_to_frames(headers, rng)
    _, est = run_device(fe, frames, np.zeros(len(frames), np.int32), np.zeros(len(frames), np.float32), payload=False,
                        want=("plsc_decoded",))
    fe.close()
    return frames[:, :90], est["plsc_decoded"]


def header_of_bits(bits64):
    return np.concatenate([np.broadcast_to(M.map_bpsk(M.SOF_BITS), bits64.shape[:-1] + (26,)), M.map_bpsk(bits64)], axis=-1)


# ------------------------------------------------------------------ 1. hard modes: bit for bit, ties included
@pytest.mark.parametrize("coherent", [1, 0])
def test_plsc_hard_modes_exact(coherent):
    rng = np.random.default_rng(100 + coherent)
    clean = np.stack([M.plheader(p) for p in range(128)])
    flipped = []
    for nflip in range(1, 21):
        for p in rng.integers(0, 128, 32):
            bits = M.CW_BITS[p] ^ M.SCR_BITS
            bits[rng.choice(64, nflip, replace=False)] ^= 1
            flipped.append(header_of_bits(bits))
    random_pm = header_of_bits(rng.integers(0, 2, (1000, 64), dtype=np.uint8))  # far from every codeword: many exact ties
    hdr = np.concatenate([clean, np.stack(flipped), random_pm])
    hdr = hdr * np.exp(1j * rng.uniform(-np.pi, np.pi, (hdr.shape[0], 1))) * rng.uniform(0.5, 2.0, (hdr.shape[0], 1))
    subset = [int(v) for v in rng.permutation(128)[:40]]  # not ascending: the ORDER of the list decides ties
    assert subset != sorted(subset)
    for enabled in (None, subset, subset + subset[:3]):
        got_in, got = decode_on_device(hdr, rng, coherent, 0, enabled)
        assert M.hard_eligible(got_in, coherent).all()  # no decision variable within float32 rounding of zero: cap 0 exclusions
        want = M.plsc_decode(got_in, coherent, 0, enabled)
        bits = M.hard_bits(got_in, coherent)[0] ^ M.SCR_BITS
        dist = np.sort((bits[:, None, :] != M.CW_BITS[None, M.enabled_order(enabled), :]).sum(-1), axis=1)
        ties = int((dist[:, 0] == dist[:, 1]).sum())
        print(f"coherent={coherent} enabled={'all' if enabled is None else len(enabled)}: {len(want)} headers, {ties} with tied minima, "
              f"{int((got != want).sum())} differ")
        assert ties > 100
        assert np.array_equal(got, want)
        if enabled is None:
            assert got[:128].tolist() == list(range(128))


# ------------------------------------------------------------------ 2. soft mode
def check_soft(x, got, enabled=None, need_all_clear=False, min_clear=0.0, what=""):
    m = M.soft_metrics(x, enabled)
    tau = M.soft_tau(x)
    top2 = np.sort(m, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > tau
    best = np.argmax(m, axis=1)
    short = m[np.arange(len(got)), got] < m.max(1) - tau
    print(f"soft {what}: {len(got)} headers, {int(clear.sum())} with margin > tau, {int(short.sum())} outside tau, "
          f"{int((got[clear] != best[clear]).sum())} clear ones differ")
    assert not short.any()
    assert np.array_equal(got[clear], best[clear])
    if need_all_clear:
        assert clear.all()
    assert clear.mean() >= min_clear
    return best


def test_plsc_soft_mode():
    rng = np.random.default_rng(7)
    # every PLSC at Es/N0 -2, 2, 10 dB, random common phase
    hdr = []
    for db in (-2.0, 2.0, 10.0):
        n0 = 10 ** (-db / 10)
        h = np.stack([M.plheader(p) for p in range(128)]) * np.exp(1j * rng.uniform(-np.pi, np.pi, (128, 1)))
        hdr.append(h + np.sqrt(n0 / 2) * (rng.normal(size=h.shape) + 1j * rng.normal(size=h.shape)))
    x, got = decode_on_device(np.concatenate(hdr), rng, 1, 1)
    best = check_soft(x, got, need_all_clear=True, what="awgn")
    assert (best[256:] == np.arange(128)).all()  # at 10 dB the model itself decodes every PLSC
    # noise only
    x, got = decode_on_device((rng.normal(size=(1000, 90)) + 1j * rng.normal(size=(1000, 90))) * M.S, rng, 1, 1)
    check_soft(x, got, min_clear=0.99, what="noise only")
    # a subset, and all-negative metrics: the never-written entries of disabled codewords (0.0) win, the first of them
    sub = [77, 3, 64]
    x, got = decode_on_device(np.concatenate(hdr), rng, 1, 1, sub)
    check_soft(x, got, sub, what="subset")
    neg = []
    for p in (0, 2, 77):
        h = M.plheader(p) * np.exp(1j * rng.uniform(-np.pi, np.pi))
        h[26:] *= -1
        neg.append(h + 0.05 * (rng.normal(size=90) + 1j * rng.normal(size=90)))
    for p, h in zip((0, 2, 77), neg):
        x, got = decode_on_device(h[None, :], rng, 1, 1, [p])
        m = M.soft_metrics(x, [p])
        assert m[0, p] < -50 and got[0] == (1 if p == 0 else 0) == np.argmax(m[0])
    # the cases of the reference's own unit test: the all-zeros PLSC in all four modes, every PLSC in the default mode
    d = M.KAT["qa_pl_signaling"]["plsc_decode"]
    h = header_of_bits(M.word_bits(int(d["scrambled_word"], 16)))[None, :]
    for coherent, soft in d["modes"]:
        assert decode_on_device(h, rng, coherent, soft)[1][0] == 0
    assert decode_on_device(np.stack([M.plheader(p) for p in range(128)]), rng, 1, 1)[1].tolist() == list(range(128))


# ------------------------------------------------------------------ 3. phases
def compare_phases(est, want, tol, keys=("sof_phase", "plheader_phase", "pilot_phase"), what=""):
    for k in keys:
        if want[k].size == 0:
            continue
        err = np.abs(M.angdiff(est[k], want[k]))
        print(f"{what} {k}: max error {err.max():.3e} rad, smallest bound {tol[k].min():.3e}, worst error / bound {np.max(err / tol[k]):.3f}")
        assert (err <= tol[k]).all(), k


@pytest.mark.parametrize("plsc,gold,nf", GEOMS)
def test_phases(plsc, gold, nf):
    rng = np.random.default_rng(1000 + plsc)
    info = M.pls_parse(plsc)
    phases = rng.uniform(-np.pi, np.pi, nf)
    phases[0] = np.pi  # the closed end of (-pi, pi]
    frames, _ = M.make_plframes(plsc, gold, nf, rng, es_n0_db=rng.uniform(0.0, 15.0), phase=phases, foffset=rng.uniform(-3e-4, 3e-4))
    cc = np.ones(nf, np.int32)
    cf = np.zeros(nf, np.float32)
    want, tol, aux = M.estimates(frames, plsc, gold, cc, cf)
    assert aux["min_quality"] >= 0.25  # |sum| >= L / 4 for every estimate: cap 0 exclusions
    fe = PlFrontEnd(gold, plsc, max_frames=nf)
    assert (fe.plframe_len, fe.n_slots, fe.n_pilots, fe.n_mod) == (info["plframe_len"], info["n_slots"], info["n_pilots"], info["n_mod"])
    _, est = run_device(fe, frames, cc, cf, payload=False)
    compare_phases(est, want, tol, what=f"plsc {plsc} gold {gold} nf {nf}")
    # the host entry gives the same numbers
    host = fe.estimate(frames, cc, cf)
    for k in est:
        assert np.array_equal(host[k], est[k]), k
    fe.close()


# ------------------------------------------------------------------ 4. fine frequency offset, 5. payload step
@pytest.mark.parametrize("plsc,gold,nf", GEOMS)
def test_fine_foffset_and_payload_step(plsc, gold, nf):
    import torch
    rng = np.random.default_rng(2000 + plsc)
    info = M.pls_parse(plsc)
    npil, flen = info["n_pilots"], info["plframe_len"]
    cc = (rng.random(nf) < 0.7).astype(np.int32)  # coarse-corrected and not, mixed in one batch
    cc[0] = 1
    if npil:
        foff = rng.uniform(-2.5e-4, 2.5e-4)
        cases = [(None, np.zeros(nf, np.float32))]
    else:
        foff = rng.uniform(-0.3, 0.3) / flen  # PLHEADER to PLHEADER: the phase runs over a whole frame
        lim = 1.0 / (2.0 * flen)
        cf = (lim * rng.choice([0.0, 0.9, -0.9, 1.1, -1.1], nf)).astype(np.float32)  # both sides of 1 / (2 plframe_len)
        cf[0] = 0
        cases = [(True, cf), (None, cf)]  # with and without the trailing header
    for with_trailing, cf in cases:
        frames, trailing = M.make_plframes(plsc, gold, nf, rng, es_n0_db=12.0, phase=rng.uniform(-np.pi, np.pi) if not npil else
                                           rng.uniform(-np.pi, np.pi, nf), foffset=foff, trailing=bool(with_trailing))
        want, tol, aux = M.estimates(frames, plsc, gold, cc, cf, trailing)
        assert (aux["wrap_margin"][want["fine_valid"] == 1] >= 0.05).all()  # no wrapped difference near +-pi: nothing to exclude
        fe = PlFrontEnd(gold, plsc, max_frames=nf + 2)
        out, est = run_device(fe, frames, cc, cf, trailing)
        what = f"plsc {plsc} gold {gold} nf {nf} trailing {bool(with_trailing)}"
        compare_phases(est, want, tol, what=what)
        # 4. fine_valid exact, fine_foffset within the sum of the phase bounds involved
        assert np.array_equal(est["fine_valid"], want["fine_valid"])
        if not npil:
            assert est["fine_valid"][-1] == (1 if with_trailing and cc[-1] and abs(cf[-1]) <= 1.0 / (2.0 * flen) else 0)
            assert (est["fine_valid"][np.abs(cf) > 1.0 / (2.0 * flen)] == 0).all()
        assert (est["fine_valid"][cc == 0] == 0).all() and (est["fine_foffset"][est["fine_valid"] == 0] == 0).all()
        ferr = np.abs(est["fine_foffset"].astype(np.float64) - want["fine_foffset"])
        print(f"{what} fine_foffset: {int(want['fine_valid'].sum())} valid, max error {ferr.max():.3e}, smallest bound "
              f"{tol['fine_foffset'].min():.3e}, worst error / bound {np.max(ferr / tol['fine_foffset']):.3f}")
        assert (ferr <= tol["fine_foffset"]).all()
        if want["fine_valid"].any():
            assert np.abs(want["fine_foffset"][want["fine_valid"] == 1] - foff).max() < 2e-5  # the estimator sees the offset put in
        assert (est["plsc_decoded"] == plsc).all()
        # 5 (i). bit for bit the payload step fed with the payload slices and the front end's own estimates
        pp = PlPayload(gold, info["n_slots"], bool(npil), max_frames=nf)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        d_pay = dev(np.ascontiguousarray(frames[:, 90:]).view(np.float32))
        inc = (2.0 * np.pi * est["fine_foffset"].astype(np.float64)).astype(np.float32)
        d_hph, d_inc, d_cc = dev(est["plheader_phase"]), dev(inc), dev(cc)
        d_pil = dev(est["pilot_phase"]) if npil else None
        d_ref = torch.zeros((nf, info["xfecframe_len"] * 2), dtype=torch.float32, device="cuda")
        capi.check(capi.lib.dvbs2_plpayload_process_device(pp._h, d_pay.data_ptr(), nf, d_hph.data_ptr(), d_inc.data_ptr(), d_cc.data_ptr(),
                                                           d_pil.data_ptr() if npil else None, d_ref.data_ptr(), None))
        torch.cuda.synchronize()
        ref = d_ref.cpu().numpy().view(np.complex64)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
        pp.close()
        # 5 (ii). against the float64 model evaluated with the MODEL's phases
        mout, bound = M.payload_step(frames, plsc, gold, cc, want, tol)
        perr = np.abs(out.astype(np.complex128) - mout)
        print(f"{what} payload: max |delta| {perr.max():.3e}, worst |delta| / bound {np.max(perr / bound):.3f}")
        assert (perr <= bound).all()
        # the host entry: same bytes
        hout, hest = fe.work(frames, cc, cf, trailing)
        assert np.array_equal(hout.view(np.uint32), out.view(np.uint32))
        for k in est:
            assert np.array_equal(hest[k], est[k]), k
        fe.close()


# ------------------------------------------------------------------ 6. end to end into the FEC chain
@pytest.mark.parametrize("modcod,short,rate,constellation,es_n0_db", [
    (4, 1, "C1_2", capi.MOD_QPSK, 6.0), (14, 0, "C3_4", capi.MOD_8PSK, 12.0)])
def test_end_to_end_into_fec_chain(modcod, short, rate, constellation, es_n0_db):
    nf, gold = 12, 5
    plsc = plsc_of(modcod, short, 1)
    framesize = capi.FECFRAME_SHORT if short else capi.FECFRAME_NORMAL
    fi = get_fec_info(capi.STANDARD_DVBS2, framesize, rate)
    m, prim = T.BCH_FIELDS[framesize]
    ob = T.OracleBch(m, prim, fi["bch_t"], fi["bch_n"])
    rng = np.random.default_rng(31 + modcod)
    sent = rng.integers(0, 256, (nf, fi["bch_k"] // 8), dtype=np.uint8)
    cw = T.ldpc_encode(fi["table"], np.unpackbits(ob.encode_bytes(sent), axis=1))
    if constellation == capi.MOD_QPSK:
        syms = ((1 - 2.0 * cw[:, 0::2]) + 1j * (1 - 2.0 * cw[:, 1::2])) * np.sqrt(0.5)
    else:
        rows = cw.shape[1] // 3
        syms = T.map_8psk(np.stack([cw[:, a:a + rows] for a in (0, rows, 2 * rows)], axis=-1))
    assert syms.shape[1] == M.pls_parse(plsc)["xfecframe_len"]
    frames, _ = M.make_plframes(plsc, gold, nf, rng, es_n0_db=es_n0_db, phase=2.1, foffset=2e-4, data=syms)
    fe = PlFrontEnd(gold, plsc, max_frames=nf)
    xfec, est = fe.work(frames, np.ones(nf, np.int32))
    assert (est["plsc_decoded"] == plsc).all() and (est["fine_valid"] == 1).all()
    assert np.abs(est["fine_foffset"] - 2e-4).max() < 2e-5
    chain = FecChain(framesize=framesize, rate=rate, constellation=constellation, group_size=4, max_frames=nf, max_trials=25)
    msg, ret, corr = chain.work(xfec, np.float32(10 ** (-es_n0_db / 10)))
    assert (ret >= 0).all() and (corr >= 0).all()
    assert np.array_equal(msg, sent)
    assert chain.fallback_rounds == 0
    chain.close()
    fe.close()


# ------------------------------------------------------------------ 7. argument checks, streams, two handles
def test_arguments_streams_and_two_handles():
    import torch
    h = C.c_void_p()
    for gold, plsc, mf, code in ((1 << 18, 4, 4, capi.EINVAL), (-1, 4, 4, capi.EINVAL), (0, 128, 4, capi.EINVAL),
                                 (0, 30 << 2, 4, capi.EINVAL), (0, 4, 0, capi.EINVAL), (0, 4, 70000, capi.EINVAL)):
        assert capi.lib.dvbs2_plframe_create(C.byref(h), gold, plsc, mf, 0) == code and not h.value
        assert capi.lib.dvbs2_last_error()
    rng = np.random.default_rng(9)
    a_plsc, b_plsc = plsc_of(4, 1, 1), plsc_of(13, 1, 0)  # two handles of different geometry alive at once
    a, b = PlFrontEnd(0, a_plsc, max_frames=4), PlFrontEnd(131071, b_plsc, max_frames=4)
    fa, _ = M.make_plframes(a_plsc, 0, 4, rng, 10.0, 0.3, 1e-4)
    fb, tb = M.make_plframes(b_plsc, 131071, 4, rng, 10.0, -1.0, 1e-6, trailing=True)
    d = torch.from_numpy(fa.view(np.float32)).cuda()
    cc = torch.ones(8, dtype=torch.int32, device="cuda")
    out = torch.zeros((4, a.xfecframe_len * 2), dtype=torch.float32, device="cuda")
    e = capi.PlFrameEstimates()
    lib = capi.lib
    assert lib.dvbs2_plframe_process_device(a._h, d.data_ptr(), 5, 0, cc.data_ptr(), None, out.data_ptr(), C.byref(e), None) == capi.ESIZE
    assert b"max_frames" in lib.dvbs2_last_error()
    assert lib.dvbs2_plframe_process_device(a._h, None, 4, 0, cc.data_ptr(), None, out.data_ptr(), C.byref(e), None) == capi.EINVAL
    assert lib.dvbs2_plframe_process_device(a._h, d.data_ptr(), 4, 0, cc.data_ptr(), None, None, None, None) == capi.EINVAL
    assert lib.dvbs2_plframe_estimate_device(a._h, d.data_ptr(), -1, 0, cc.data_ptr(), None, None, None) == capi.EINVAL
    # a pilotless handle needs coarse_foffset
    db = torch.from_numpy(np.concatenate([fb.reshape(-1), tb]).view(np.float32)).cuda()
    assert lib.dvbs2_plframe_estimate_device(b._h, db.data_ptr(), 4, 1, cc.data_ptr(), None, C.byref(e), None) == capi.EINVAL
    assert b"coarse_foffset" in lib.dvbs2_last_error()
    with pytest.raises(ValueError):
        b.estimate(fb, np.ones(4, np.int32))
    # subset index >= 128 (reference lib/reed_muller.cc:48-52)
    bad = np.array([0, 64, 128], np.uint8)
    assert lib.dvbs2_plframe_set_expected_pls(a._h, bad.ctypes.data, 3) == capi.EINVAL and b"128" in lib.dvbs2_last_error()
    assert lib.dvbs2_plframe_set_expected_pls(a._h, None, 3) == capi.EINVAL
    ok = np.array([0, 64, 127], np.uint8)
    assert lib.dvbs2_plframe_set_expected_pls(a._h, ok.ctypes.data, 3) == capi.OK
    a.set_expected_pls([])
    # the Python class refuses what it would have to reinterpret
    with pytest.raises(TypeError):
        a.work(fa.astype(np.complex128), np.ones(4, np.int32))
    with pytest.raises(ValueError):
        a.work(fa[:, :-1], np.ones(4, np.int32))
    with pytest.raises(ValueError):
        a.work(fa[:, ::-1], np.ones(4, np.int32))
    with pytest.raises(ValueError):
        a.work(fa, np.ones(3, np.int32))
    # both handles, each on a stream of its own, after the failed calls: still right
    cca, ccb, cfb = np.ones(4, np.int32), np.ones(4, np.int32), np.zeros(4, np.float32)
    oa, ea = run_device(a, fa, cca, stream=torch.cuda.Stream())
    ob, eb = run_device(b, fb, ccb, cfb, tb, stream=torch.cuda.Stream())
    oa0, ea0 = run_device(a, fa, cca)
    assert np.array_equal(oa.view(np.uint32), oa0.view(np.uint32)) and all(np.array_equal(ea[k], ea0[k]) for k in ea)
    for fe, f, c, cf, t, est, plsc, gold in ((a, fa, cca, None, None, ea, a_plsc, 0), (b, fb, ccb, cfb, tb, eb, b_plsc, 131071)):
        want, tol, _ = M.estimates(f, plsc, gold, c, cf if cf is not None else np.zeros(4), t)
        compare_phases(est, want, tol, what=f"plsc {plsc}")
        assert np.array_equal(est["fine_valid"], want["fine_valid"]) and (est["plsc_decoded"] == plsc).all()
        assert (np.abs(est["fine_foffset"] - want["fine_foffset"]) <= tol["fine_foffset"]).all()
    # n_frames = 0 is a no-op
    assert lib.dvbs2_plframe_process_device(a._h, None, 0, 0, None, None, None, None, None) == capi.OK
    a.close()
    b.close()
