"""Coarse frequency offset estimate (dvbs2_plcoarse_*) and rotator (dvbs2_rotator_*) on the device against the float64 model
of tests/plcoarse_model.py: every estimate within the bound the model derives for a float32 evaluation on every eligible
window, new_est and coarse_corrected exactly there; the rotator within its derived per-sample bound, and bit for bit against
itself however the stream is cut or placed; and both in the pipeline PlSync -> PlCoarse -> Rotator -> PlFrontEnd -> FecChain
on a stream with a carrier offset. Every input set is vouched for by tests/test_plcoarse_model.py. Both are UNPINNED against
the genuine reference (VOLK and gr::fast_atan2f are not part of the reference tree)."""
import ctypes as C

import numpy as np
import pytest

import plcoarse_model as K
import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import FecChain, PlCoarse, PlFrontEnd, PlSync, Rotator, capi

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def device_frames(pc, x, plscs, fixed=False):
    """one work_device() over back-to-back rows; returns the three output arrays"""
    import torch
    n = x.shape[0]
    d_x, d_p = dev(x), dev(np.asarray(plscs, np.uint8))
    d_f = torch.full((n,), -9.0, dtype=torch.float32, device="cuda")
    d_c = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    d_n = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    pc.work_device(d_x.data_ptr(), x.shape[1], n, 0 if fixed else d_p.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_n.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(coarse_foffset=d_f.cpu().numpy(), coarse_corrected=d_c.cpu().numpy(), new_est=d_n.cpu().numpy())


def compare(got, m, what):
    """the comparison the whole file uses; returns (windows, ineligible windows)"""
    idx, n_win, n_bad = K.comparable(m)
    # the bound of an estimate holds until the next one replaces it
    bound = np.maximum.accumulate(np.where(m["new_est"] > 0, 1, 0) * np.arange(len(m["bound"])))
    bound = m["bound"][bound]
    err = np.abs(got["coarse_foffset"][idx].astype(np.float64) - m["foffset"][idx])
    worst = float((err / np.maximum(bound[idx], 1e-300)).max()) if len(idx) and m["new_est"][idx].any() else 0.0
    print(f"{what}: {n_win} windows, {n_bad} ineligible, {len(idx)} frames compared, largest error {err.max() if len(idx) else 0:.2e}, "
          f"largest error / bound {worst:.3f}")
    assert (err <= bound[idx]).all(), what
    assert got["new_est"][idx].tolist() == m["new_est"][idx].tolist(), what
    assert got["coarse_corrected"][idx].tolist() == m["corrected"][idx].tolist(), what
    return n_win, n_bad


# ------------------------------------------------------------------ 1. estimator values
def test_qa_cases_of_the_reference():
    for full in (False, True):
        pc1 = PlCoarse(1, K.QA_PLSC if full else -1, max_frames=8)
        pc2 = PlCoarse(2, K.QA_PLSC if full else -1, max_frames=8)
        for f in K.QA_OFFSETS + K.QA_CORRECTED:
            pc1.reset()
            x = K.qa_unit_period(f)
            got = device_frames(pc1, x, [K.QA_PLSC], fixed=full)
            assert compare(got, K.run(x, [K.QA_PLSC], 1, full), f"qa unit {f} full={full}")[1] == 0
            # the reference's own tolerances hold for the device too (they are far wider than the bound)
            assert abs(got["coarse_foffset"][0] - f) <= (5e-3 if abs(f) < K.RANGE else 1e-5) * abs(f)
            assert got["coarse_corrected"][0] == int(abs(f) < K.RANGE)
        for f in K.QA_OFFSETS:
            pc2.reset()
            x = K.qa_period_two(f)
            got = device_frames(pc2, x, [K.QA_PLSC] * 4, fixed=full)
            assert compare(got, K.run(x, [K.QA_PLSC] * 4, 2, full), f"qa period 2 {f} full={full}")[1] == 0
            assert got["new_est"].tolist() == [0, 1, 0, 1]
        pc1.close()
        pc2.close()


@pytest.mark.parametrize("name,seed,n,es,cap", K.RANDOM_SETS, ids=[s[0] for s in K.RANDOM_SETS])
def test_random_sets(name, seed, n, es, cap):
    for period in K.PERIODS:
        x, plscs = K.random_set(seed, n, es, period)
        for known in (False, True):
            # a known-PLSC handle takes the full PLHEADER throughout; the per-frame PLSC array still names each header
            pc = PlCoarse(period, 0 if known else -1, max_frames=n)
            got = device_frames(pc, x, plscs)
            n_win, n_bad = compare(got, K.run(x, plscs, period, known), f"{name} period {period} {'full' if known else 'sof'}")
            assert n_bad <= cap * n_win
            pc.close()


def test_host_entry_equals_the_device_entry():
    x, plscs = K.random_set(5, 40, 10.0, 5)
    pc = PlCoarse(5, -1, max_frames=64)
    a = device_frames(pc, x, plscs)
    pc.reset()
    wide = np.zeros((40, 131), np.complex64)  # a stride that is not the header length
    wide[:, :90] = x
    b = pc.work(wide, plscs)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    pc.close()


# ------------------------------------------------------------------ 2. mode switching
def test_mode_follows_the_state_as_in_the_model():
    x, plscs = K.mode_switch_set()
    m = K.run(x, plscs, 1)
    assert m["full"].tolist() == [0] * 5 + [1] * 6 + [0] * 4  # SOF -> full -> SOF
    pc = PlCoarse(1, -1, max_frames=32)
    got = device_frames(pc, x, plscs)
    assert compare(got, m, "mode switch") == (15, 0)
    assert got["coarse_corrected"].tolist() == [0] * 4 + [1] * 6 + [0] * 5
    # on every frame the estimate of the OTHER form lies outside the bound around the model's: had the device taken the other
    # form anywhere, the comparison above would have failed there
    for i in range(len(plscs)):
        other = K.run(x[i:i + 1], plscs[i:i + 1], 1, known_plsc=not m["full"][i])
        assert abs(other["foffset"][0] - m["foffset"][i]) > m["bound"][i], i
    pc.close()


# ------------------------------------------------------------------ 3. streaming, and the two ways to address headers
def test_split_calls_and_both_addressing_forms_give_the_same_bits():
    import torch
    x, plscs = K.streaming_set()
    n = x.shape[0]
    pc = PlCoarse(4, -1, max_frames=64)
    one = device_frames(pc, x, plscs)
    assert compare(one, K.run(x, plscs, 4), "streaming, one call")[1] == 0
    pc.reset()
    parts = [device_frames(pc, x[a:b], plscs[a:b]) for a, b in ((0, 1), (1, 8), (8, n))]
    for k in one:
        assert np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint32), one[k].view(np.uint32)), k
    # the same headers inside a raw buffer, named by PlSync's records (absolute indices, buffer base 1000)
    pc.reset()
    rng = np.random.default_rng(9)
    gaps = rng.integers(0, 40, n)
    buf, recs, pos = [], np.zeros(n + 2, PlSync.FRAME_DTYPE), 0
    for i in range(n):
        buf.append(P.qpsk(rng, int(gaps[i])).astype(np.complex64))
        pos += int(gaps[i])
        recs[i] = (1000 + pos, 0.0, plscs[i], 3, (0, 0))
        buf.append(x[i])
        pos += 90
    raw = np.concatenate(buf)
    recs[n] = (1000 + raw.size - 89, 0.0, 5, 3, (0, 0))  # a header that leaves the buffer: passed over
    recs[n + 1] = (999, 0.0, 5, 3, (0, 0))               # ... and one that starts before it
    d_raw, d_rec = dev(raw), torch.from_numpy(recs.view(np.uint8)).cuda()
    d_f = torch.full((n + 2,), -9.0, dtype=torch.float32, device="cuda")
    d_c = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda")
    d_n = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda")
    pc.work_records_device(d_raw.data_ptr(), raw.size, 1000, d_rec.data_ptr(), n + 2, d_f.data_ptr(), d_c.data_ptr(), d_n.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dict(coarse_foffset=d_f.cpu().numpy(), coarse_corrected=d_c.cpu().numpy(), new_est=d_n.cpu().numpy())
    for k in one:
        assert np.array_equal(got[k][:n].view(np.uint32), one[k].view(np.uint32)), k
        assert got[k][n] == got[k][n + 1] == (0 if k == "new_est" else one[k][-1])  # the state, repeated
    pc.close()


# ------------------------------------------------------------------ 4. rotator
def device_rotate(rot, x, in_place=False, d_x=None):
    import torch
    d_x = dev(x) if d_x is None else d_x
    d_y = d_x if in_place else torch.zeros_like(d_x)
    rot.work_device(d_x.data_ptr(), x.size, d_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_y.cpu().numpy().view(np.complex64)


def rand_syms(seed, n):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=n) + 1j * rng.normal(size=n)) * rng.uniform(0.2, 4.0)).astype(np.complex64)


def check_rotation(got, want, bound, what):
    err = np.abs(got.astype(np.complex128) - want)
    print(f"{what}: largest error {err.max():.2e}, largest error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("inc", [1e-7, -3e-5, 0.0123, -1.0, 2.5, np.pi, -np.pi, 7.0])
def test_rotator_accuracy_over_increments_and_far_out(inc):
    n = 6001
    x = rand_syms(int(abs(inc) * 1e7) % 9973, n)
    rot, mod = Rotator(inc), K.Rotator(inc)
    for seek in (0, 123456789, (1 << 40) - 123456789 - 2 * n):  # the third call ends at 2^40 + n
        rot.seek(seek)
        mod.seek(seek)
        want, bound = mod.work(x)
        check_rotation(device_rotate(rot, x), want, bound, f"inc {inc} from sample {mod.counter - n}")
    assert rot.position() == (mod.counter, 0) and mod.counter == (1 << 40) + n
    rot.close()


def test_rotator_schedules():
    n = 5000
    x = rand_syms(3, 3 * n)
    rot, mod = Rotator(0.01), K.Rotator(0.01)
    ups = [(700, -0.3), (701, 0.25), (2000, 1e-4), (2000, -2.0),           # inside the first call; an equal pair: -2.0 wins
           (n, 0.7),                                                       # exactly at the end of the first call
           (n + 10, 0.1), (n + 11, 0.2), (n + 12, 0.3), (n + 13, 0.4), (n + 14, 0.5), (n + 15, 0.6), (n + 16, 0.7),
           (n + 17, 0.8), (n + 18, 0.9), (n + 19, 1.0),                   # more segments than one launch takes
           (2 * n + 300, -0.05), (10 * n, 3.0)]                            # in the third call; beyond every call
    for off, inc in ups:
        rot.schedule(off, inc)
        mod.schedule(off, inc)
    outs = []
    for c in range(3):
        if c == 1:
            rot.schedule(100, 9.9)  # already behind the counter: dropped when the call reaches it
            mod.schedule(100, 9.9)
        if c == 2:
            rot.set_phase_inc(-0.002)  # at once
            mod.set_phase_inc(-0.002)
        want, bound = mod.work(x[c * n:(c + 1) * n])
        got = device_rotate(rot, x[c * n:(c + 1) * n])
        check_rotation(got, want, bound, f"schedule, call {c}")
        outs.append(got)
        assert rot.position() == (mod.counter, len(mod.queue))
    assert mod.dropped == 1 and len(mod.queue) == 1
    rot.reset()
    mod.reset()
    assert rot.position() == (0, 0)
    want, bound = mod.work(x[:64])
    check_rotation(device_rotate(rot, x[:64]), want, bound, "after reset")
    rot.close()


def test_rotator_is_bit_exact_however_it_is_cut_or_placed():
    import torch
    n = 40003
    x = rand_syms(8, n)
    ups = [(1234, 0.3), (20001, -0.004), (20002, 2.0), (39999, 1e-3)]

    def fresh():
        r = Rotator(0.0371)
        for off, inc in ups:
            r.schedule(off, inc)
        return r
    r = fresh()
    whole = device_rotate(r, x)
    r.close()
    # in place
    r = fresh()
    assert np.array_equal(device_rotate(r, x, in_place=True).view(np.uint32), whole.view(np.uint32))
    r.close()
    # unequal pieces, odd starts (8-byte but not 16-byte aligned pieces), cuts on and next to the updates
    r = fresh()
    cuts = [0, 1, 8, 1234, 1235, 7777, 20001, 20002, 33333, n]
    pieces = [device_rotate(r, x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(pieces).view(np.uint32), whole.view(np.uint32))
    r.close()
    # input and output at different 16-byte phases (the 8-byte path), and both at an odd symbol
    d_big = torch.zeros(2 * (n + 2), device="cuda")
    d_x = dev(x)
    for in_off, out_off in ((0, 1), (1, 1)):
        r = fresh()
        d_in = torch.zeros(2 * (n + 1), device="cuda")
        d_in[2 * in_off:2 * (in_off + n)] = d_x
        r.work_device(d_in.data_ptr() + 8 * in_off, n, d_big.data_ptr() + 8 * out_off, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_big.cpu().numpy()[2 * out_off:2 * (out_off + n)].view(np.complex64)
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), (in_off, out_off)
        r.close()
    # the host entry
    r = fresh()
    assert np.array_equal(r.work(x).view(np.uint32), whole.view(np.uint32))
    r.close()


# ------------------------------------------------------------------ 5. end to end
def run_pipeline(x, sofs, plsc, sent, rotate):
    import torch
    e = P.E2E["e2e-qpsk"]
    st = torch.cuda.current_stream().cuda_stream
    L = M.pls_parse(plsc)["plframe_len"]
    ps = PlSync(plsc=plsc, max_symbols=max(x.size, PlSync.MIN_SYMBOLS), max_frames=64)
    d_x = dev(x)
    d_rec = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
    ps.work_device(d_x.data_ptr(), x.size, d_rec.data_ptr(), st)
    nf, consumed, state = ps.finish()
    recs = d_rec.cpu().numpy().view(PlSync.FRAME_DTYPE)[:nf]
    assert recs["sof_index"].tolist() == sofs and state == capi.PLSYNC_LOCKED
    # pass 1: the estimator on the records of the raw buffer (base 0: the first search of this handle)
    pc = PlCoarse(K.E2E_PERIOD, plsc, max_frames=64)
    d_f = torch.zeros(nf, dtype=torch.float32, device="cuda")
    pc.work_records_device(d_x.data_ptr(), x.size, 0, d_rec.data_ptr(), nf, d_f.data_ptr(), 0, 0, st)
    torch.cuda.synchronize()
    f = float(d_f.cpu().numpy()[-1])
    p1, f_model, _ = K.e2e_model(x, sofs, plsc)
    print(f"pass 1: device {f:.6e}, model {f_model:.6e}, bound {p1['bound'].max():.1e}, true {K.E2E_FOFFSET}")
    assert abs(f - f_model) <= p1["bound"].max()
    if rotate:
        rot = Rotator(-2.0 * np.pi * f)
        rot.work_device(d_x.data_ptr(), x.size, d_x.data_ptr(), st)
        rot.close()
    locked = [int(r["sof_index"]) for r in recs if r["flags"] & 2]
    assert len(locked) >= len(sofs) - 1  # the first header only takes the tracker to `found`
    d_fr = torch.zeros(2 * (len(locked) * L + 90), dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ps.gather_device(d_x.data_ptr(), d_rec.data_ptr(), nf, plsc, d_fr.data_ptr(), d_cnt.data_ptr(), st)
    torch.cuda.synchronize()
    cnt = int(d_cnt.item())
    assert cnt == len(locked)
    # pass 2: the estimator on the gathered frames; its coarse_corrected array is the front end's input
    pc2 = PlCoarse(1, plsc, max_frames=64)
    d_cc = torch.zeros(cnt, dtype=torch.int32, device="cuda")
    d_f2 = torch.zeros(cnt, dtype=torch.float32, device="cuda")
    pc2.work_device(d_fr.data_ptr(), L, cnt, 0, d_f2.data_ptr(), d_cc.data_ptr(), 0, st)
    fe = PlFrontEnd(P.E2E_GOLD, plsc, max_frames=cnt)
    d_xfec = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
    fe.work_device(d_fr.data_ptr(), cnt, 1, d_cc.data_ptr(), d_f2.data_ptr(), d_xfec.data_ptr(), st)
    torch.cuda.synchronize()
    print(f"pass 2: estimates {d_f2.cpu().numpy()}, coarse_corrected {d_cc.cpu().tolist()}")
    chain = FecChain(framesize=capi.FECFRAME_SHORT, rate=e["rate"], constellation=capi.MOD_QPSK, group_size=4, max_frames=cnt, max_trials=25)
    msg, ret, corr = chain.work(d_xfec.cpu().numpy().view(np.complex64), np.float32(10 ** (-K.E2E_ES_N0_DB / 10)))
    which = [sofs.index(s) for s in locked]
    for o in (chain, fe, pc2, pc, ps):
        o.close()
    return d_cc.cpu().numpy(), msg, ret, sent[which]


def test_end_to_end_with_a_carrier_offset():
    x, sofs, sent, plsc = K.e2e_stream()
    cc, msg, ret, want = run_pipeline(x, sofs, plsc, sent, rotate=True)
    assert cc.all() and (ret >= 0).all()
    assert np.array_equal(msg, want)  # every frame's BBFRAME
    # the same pipeline without the rotator does not decode: the comparison above can fail
    cc, msg, ret, want = run_pipeline(x, sofs, plsc, sent, rotate=False)
    assert not cc.any()
    assert not any(np.array_equal(a, b) for a, b in zip(msg, want))


# ------------------------------------------------------------------ 6. arguments
def test_arguments():
    lib, h = capi.lib, C.c_void_p()
    for period, plsc, mf in ((0, -1, 8), (1, -2, 8), (1, 128, 8), (1, -1, 0)):
        assert lib.dvbs2_plcoarse_create(C.byref(h), period, plsc, mf, 0) == capi.EINVAL and not h.value
        assert lib.dvbs2_last_error()
    pc = PlCoarse(1, -1, max_frames=4)
    with pytest.raises(TypeError):
        pc.work(np.zeros((2, 90), np.complex128), [0, 0])
    with pytest.raises(ValueError):
        pc.work(np.zeros((2, 89), np.complex64), [0, 0])
    with pytest.raises(ValueError):
        pc.work(np.zeros((2, 90), np.complex64))  # no fixed PLSC and none given
    with pytest.raises(ValueError):
        pc.work(np.zeros((5, 90), np.complex64), [0] * 5)  # beyond max_frames
    assert lib.dvbs2_plcoarse_estimate_device(pc._h, 8, 90, None, 1, None, None, None, None) == capi.EINVAL  # no PLSC
    assert lib.dvbs2_plcoarse_estimate_device(pc._h, 8, 89, 8, 1, None, None, None, None) == capi.EINVAL
    assert lib.dvbs2_plcoarse_estimate_device(pc._h, 8, 90, 8, 5, None, None, None, None) == capi.ESIZE
    pc.close()
    assert lib.dvbs2_rotator_create(C.byref(h), float("nan"), 0) == capi.EINVAL and not h.value
    rot = Rotator(0.1)
    with pytest.raises(TypeError):
        rot.work(np.zeros(4, np.complex128))
    with pytest.raises(ValueError):
        rot.work(np.zeros((2, 2), np.complex64))
    assert lib.dvbs2_rotator_schedule(rot._h, -1, 0.1) == capi.EINVAL
    assert lib.dvbs2_rotator_set_phase_inc(rot._h, float("inf")) == capi.EINVAL
    assert lib.dvbs2_rotator_seek(rot._h, -1) == capi.EINVAL
    assert lib.dvbs2_rotator_rotate_device(rot._h, 4, 1, 8, None) == capi.EINVAL  # a 4-byte aligned address
    assert rot.position() == (0, 0)
    rot.close()
