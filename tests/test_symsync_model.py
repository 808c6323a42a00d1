"""Symbol timing recovery without a device: the two models of tests/symsync_model.py against the MATLAB vectors the reference's
own QA quotes (tests/golden/symsync_kat.json), its open-loop and tag-placement cases; the host-only entries of the library
against the model; the properties of the RRC bank; and restatement (b) -- the device's arithmetic -- against the float64 model
(a) on every closed-loop input the GPU tests use."""
import numpy as np
import pytest

import symsync_model as S
from dvbs2rx_amd import symsync_geometry, symsync_loop_constants, symsync_taps


@pytest.mark.parametrize("exact", [True, False], ids=["float64", "device-arithmetic"])
def test_matlab_vectors_to_the_reference_places(exact):
    for v, x, want in S.kat_vectors():
        out, idx, mu, consumed, status = S.SymSync(exact=exact, **S.kat_cfg(v)).work(x)
        assert status == 0 and out.size == want.size == 49, v["name"]
        d = np.asarray(out, np.complex128) - want
        print(v["name"], "largest difference", max(np.abs(d.real).max(), np.abs(d.imag).max()))
        assert (np.round(d.real, S.KAT["places"]) == 0).all() and (np.round(d.imag, S.KAT["places"]) == 0).all(), v["name"]


@pytest.mark.parametrize("exact", [True, False], ids=["float64", "device-arithmetic"])
@pytest.mark.parametrize("interp", [1, 2, 3])
def test_open_loop_reproduces_its_symbols(exact, interp):
    x, syms = S.open_loop_input()
    m = S.SymSync(sps=2, damping=0.0, interp_method=interp, exact=exact)
    assert m.K1 == 0 and m.K2 == 0
    if interp == 1:
        # all symbols but the first: the synchronizer needs two symbols to start
        want = syms[1:]
    else:
        # at mu = 0 the reference's Farrow expressions return in[m_k - 1], the sample BEFORE the basepoint (:43-45, :63-65):
        # with the symbols one sample later they come out exactly, the first included
        x = np.roll(x, 1)
        want = syms[:6]
    out, idx, mu, consumed, status = m.work(x)
    assert np.array_equal(np.asarray(out, np.complex128), want.astype(np.complex128))
    assert (mu == 0).all() and idx.tolist() == list(range(2, 14, 2)) and consumed == 14


def test_tag_placement():
    t = S.KAT["tags"]
    sps, nsyms = t["sps"], t["nsyms"]
    rng = np.random.default_rng(1)
    a = (((1 - 2.0 * rng.integers(0, 2, nsyms)) + 1j * (1 - 2.0 * rng.integers(0, 2, nsyms))) * np.sqrt(0.5)).astype(np.complex64)
    x = np.zeros(nsyms * sps, np.complex64)
    x[::sps] = a
    m = S.SymSync(sps=sps, damping=t["damping"], interp_method=1)
    out, idx, mu, consumed, status = m.work(x)
    assert np.array_equal(out[:2], a[1:3])
    tags = list(range(0, x.size, t["tag_period"]))
    placed, pending = S.map_tag_offsets(tags, 0, idx + m.H, 0, m.H)  # strobe indices relative to the buffer with its history
    want = [0] + list(range(1, nsyms - 1, 2))
    assert placed == want[:len(placed)] and len(placed) >= len(want) - 1
    # in two calls, with a tag left pending between them
    m.reset()
    cut = 22
    o1, i1, _, c1, _ = m.work(x[:cut])
    p1, pend = S.map_tag_offsets([g for g in tags if g < c1], 0, i1 + m.H, 0, m.H)
    o2, i2, _, c2, _ = m.work(x[c1:])
    p2, pend2 = S.map_tag_offsets(pend + [g for g in tags if c1 <= g < c1 + c2], c1, i2 - c1 + m.H, o1.size, m.H)
    assert p1 + p2 == placed and np.array_equal(np.concatenate([o1, o2]), out)


CFGS = [(2, 0.01, 1.0, 0.2), (4, 0.005, 0.707, 0.35), (2, 0.001, 1.0, 0.2), (8, 0.05, 2.0, 0.05), (2, 0.01, 0.0, 0.2), (2, 3.0, 1.0, 0.2)]


def test_library_constants_and_geometry_equal_the_model():
    for sps, bw, damp, ro in CFGS:
        got, want = symsync_loop_constants(sps, bw, damp, ro), S.loop_constants(sps, bw, damp, ro)
        assert [float(g) for g in got] == [float(w) for w in want], (sps, bw, damp, ro, got, want)
    assert symsync_loop_constants(2, 0.01, 0.0, 0.2)[1:] == (0.0, 0.0)
    for sps in (2, 4, 8):
        for delay in (3, 5, 10):
            for interp in range(4):
                assert symsync_geometry(sps, delay, 128, interp) == S.geometry(sps, delay, 128, interp)
    assert symsync_geometry(2, 5, 128, 0) == (21, 10, 21) and symsync_geometry(4, 5, 128, 0) == (41, 20, 42)
    assert symsync_geometry(2, 5, 128, 1)[2] == 2 and symsync_geometry(4, 5, 128, 3)[2] == 5


@pytest.mark.parametrize("sps,ro,delay,ns", [(2, 0.2, 5, 128), (4, 0.35, 5, 128), (2, 0.25, 8, 32), (2, 0.05, 5, 64)])
def test_bank(sps, ro, delay, ns):
    lib, mod = symsync_taps(sps, ro, delay, ns), S.taps(sps, ro, delay, ns)
    L = 2 * sps * delay + 1
    assert lib.shape == mod.shape == (ns, L)
    # two double evaluations of the same closed form, each rounded to float32 once
    assert np.abs(lib.astype(np.float64) - mod).max() <= 2.0 ** -23 * np.abs(mod).max()
    b = lib.astype(np.float64)
    assert abs(b.sum() - ns) <= np.abs(b).sum() * S.U  # the prototype sums to the gain
    assert np.array_equal(lib[0], lib[0, ::-1])         # subfilter 0: symmetric about its centre tap
    assert (lib[1:, 0] == 0).all()                      # the zero padding, flipped to the front
    assert np.array_equal(lib[ns // 2, 1:], lib[ns // 2, :0:-1])  # the half-sample subfilter: symmetric between two taps
    for i in (1, 3, ns // 4):                           # subfilter i mirrors subfilter n_subfilt - i
        assert np.abs(lib[i, 1:] - lib[ns - i, :0:-1]).max() <= 2.0 ** -23 * np.abs(mod).max()


@pytest.mark.parametrize("sps,ro,delay", [(2, 0.2, 5), (4, 0.35, 5), (2, 0.2, 10)])
def test_rrc_pair_has_no_intersymbol_interference(sps, ro, delay):
    n = np.arange(-delay * sps, delay * sps + 1)
    p = S.rrc(n / sps, ro)
    g = np.convolve(p, p)
    c = g.size // 2
    # g_truncated(k) - g_full(k) = - sum over pairs with an index outside the window, at most 2 max|p| (l1 tail of p); the
    # untruncated pair is a Nyquist pulse sampled above its bandwidth, so g_full is zero at every other symbol instant
    # the l1 tail of p, summed out to 4000 symbols (it falls as 1 / t^2: what lies beyond is below 1e-3 of the sum)
    far = np.arange(delay * sps + 1, 4000 * sps)
    tail = 2.0 * np.abs(S.rrc(far / sps, ro)).sum() * 1.001
    tol = 2.0 * np.abs(p).max() * tail / g[c]
    isi = np.abs(g[c % sps::sps] / g[c])
    k = np.arange(isi.size) - c // sps
    print(f"sps {sps} rolloff {ro} delay {delay}: largest ISI {isi[k != 0].max():.2e}, tolerance {tol:.2e}")
    assert abs(g[c] / sps - 1.0) <= tol and (isi[k != 0] <= tol).all()


@pytest.mark.parametrize("name", [c[0] for c in S.CLOSED_SETS])
def test_restatement_against_the_float64_model(name):
    cfg, x = S.closed_set(name)
    a, b = S.SymSync(exact=True, **cfg), S.SymSync(exact=False, **cfg)
    oa, ia, ma, ca, sa = a.work(x)
    ob, ib, mb, cb, sb = b.work(x)
    assert sa == sb == 0 and ca == cb and np.array_equal(ia, ib)  # the strobe indices are equal
    assert len(set(np.diff(ia).tolist())) >= 2                    # the loop did adjust its jumps
    dmu = np.abs(ma - mb).max()
    bound = S.output_bound(a)
    err = np.maximum(np.abs(oa.real - ob.real), np.abs(oa.imag - ob.imag))
    frac = cfg["n_subfilt"] * ma
    near = (np.abs(frac - np.round(frac)) <= S.GUARD) if cfg["interp_method"] == 0 else np.zeros(ma.size, bool)
    print(f"{name}: {oa.size} strobes, jumps {sorted(set(np.diff(ia).tolist()))}, largest mu difference {dmu:.2e} at {np.abs(ma - mb).argmax()}, "
          f"largest output difference {err[~near].max():.2e}, largest difference / bound {(err[~near] / bound[~near]).max():.3f}, "
          f"guarded {near.mean():.3%}")
    assert dmu <= S.mu_tol(name)
    assert (err[~near] <= bound[~near]).all()
    assert near.mean() <= S.GUARD_SHARE


def test_stop_case_of_the_gpu_tests_stops_in_the_model():
    x = S.qpsk_stream(**S.STOP_STREAM)[0]
    m = S.SymSync(**S.STOP_CFG)
    out, idx, mu, consumed, status = m.work(x)
    print("stop case: status", status, "after", out.size, "symbols, consumed", consumed)
    assert status == 1 and 0 < out.size < x.size // 4
    assert m.work(x[consumed:])[3:] == (0, 1)  # a stopped stream returns at once


def test_create_refuses_bad_arguments_before_it_looks_for_a_device():
    import ctypes as C
    from dvbs2rx_amd import capi
    h = C.c_void_p()
    good = dict(sps=2, loop_bw=0.01, damping=1.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp=0, max_streams=1, max_samples=1024)
    for bad in (dict(sps=3), dict(sps=0), dict(interp=4), dict(interp=-1), dict(rolloff=1.5), dict(loop_bw=float("nan")), dict(n_subfilt=1),
                dict(n_subfilt=4096),               # 4096 x 21 floats: the bank does not fit the LDS
                dict(sps=8, rrc_delay=64),          # a history of 1028 samples does not fit the ring
                dict(max_streams=0), dict(max_samples=1)):
        a = dict(good, **bad)
        rc = capi.lib.dvbs2_symsync_create(C.byref(h), a["sps"], a["loop_bw"], a["damping"], a["rolloff"], a["rrc_delay"], a["n_subfilt"], a["interp"],
                                           a["max_streams"], a["max_samples"], 0)
        assert rc == capi.EINVAL and not h.value and capi.lib.dvbs2_last_error(), bad
    # the same bank is acceptable to a Farrow interpolator, which keeps no bank in LDS: the geometry alone is not refused
    assert symsync_geometry(2, 5, 4096, 1) == (21, 10, 2)
