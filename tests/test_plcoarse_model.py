"""CPU tests of the coarse frequency offset estimate and the rotator: the float64 model of plcoarse_model.py against what the
reference recorded about itself (lib/qa_pl_freq_sync.cc:61-172, with that file's own tolerances), the library's host-only
entries against the model, the rotator's schedule semantics on the model, and the check -- with the model alone -- that every
input set the GPU tests run stays inside its cap of windows a float32 evaluation may decide differently."""
import numpy as np
import pytest

import plcoarse_model as K
import plframe_model as M

PLCOARSE = ("create", "destroy", "reset", "estimate_device", "estimate_records_device", "estimate", "weights")
ROTATOR = ("create", "destroy", "reset", "set_phase_inc", "schedule", "seek", "position", "rotate_device", "rotate", "measure")


# ------------------------------------------------------------------ the library's host-only side
def test_library_exports_the_new_entries():
    from dvbs2rx_amd import capi
    for prefix, names in (("dvbs2_plcoarse_", PLCOARSE), ("dvbs2_rotator_", ROTATOR)):
        for name in names:
            assert hasattr(capi.lib, prefix + name), prefix + name
            assert prefix + name in capi.SYMBOLS


def test_window_weights_equal_the_model():
    import dvbs2rx_amd
    for full, L in ((True, 89), (False, 25)):
        w = dvbs2rx_amd.plcoarse_weights(full)
        want = K.weights(full)
        assert w.dtype == np.float32 and w.shape == (L,)
        assert np.array_equal(w, want.astype(np.float32))  # the same expression in double, rounded once
        assert abs(float(want.sum()) - 1.0) < 1e-12        # the window of an unbiased estimator


# ------------------------------------------------------------------ the reference's own unit tests, on the model
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("f", K.QA_OFFSETS)
def test_qa_unit_period(f, full):
    m = K.run(K.qa_unit_period(f), [K.QA_PLSC], 1, known_plsc=full)
    assert m["new_est"].tolist() == [1] and m["corrected"].tolist() == [0] and m["full"].tolist() == [int(full)]
    assert abs(m["foffset"][0] - f) <= 1e-6 * abs(f)  # BOOST_CHECK_CLOSE(.., 1e-4 %)
    assert m["eligible"].all()


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("f", K.QA_OFFSETS)
def test_qa_period_two(f, full):
    m = K.run(K.qa_period_two(f), [K.QA_PLSC] * 4, 2, known_plsc=full)
    assert m["new_est"].tolist() == [0, 1, 0, 1] and not m["corrected"].any()
    assert m["foffset"][0] == 0.0                      # nothing estimated yet
    assert abs(m["foffset"][1] - f) <= 1e-6 * abs(f)
    assert m["foffset"][2] == m["foffset"][1]          # the latest estimate stands until the next window ends
    assert abs(m["foffset"][3] + f) <= 1e-6 * abs(f)   # the accumulator restarted: nothing of the first pair is left
    assert m["eligible"].all()


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("f", K.QA_CORRECTED)
def test_qa_coarse_corrected_state(f, full):
    assert abs(f) < K.RANGE
    m = K.run(K.qa_unit_period(f), [K.QA_PLSC], 1, known_plsc=full)
    assert m["new_est"].tolist() == [1] and m["corrected"].tolist() == [1]
    assert abs(m["foffset"][0] - f) <= 5e-3 * abs(f)   # BOOST_CHECK_CLOSE(.., 0.5 %)


def test_mode_follows_the_state():
    x, plscs = K.mode_switch_set()
    m = K.run(x, plscs, 1)
    # SOF while not corrected; the 5th frame (first small offset) is still estimated on the SOF and sets the state
    assert m["full"].tolist() == [0] * 5 + [1] * 6 + [0] * 4
    assert m["corrected"].tolist() == [0] * 4 + [1] * 6 + [0] * 5
    assert m["eligible"].all()
    # a handle that knows the PLSC uses the full PLHEADER throughout
    assert K.run(x, plscs, 1, known_plsc=True)["full"].all()


# ------------------------------------------------------------------ rotator schedule semantics
def rot_incs(r, n):
    return [(s, ln, inc) for s, ln, _, inc, _ in r.segments(n)]


def test_rotator_schedule_semantics():
    a, b, c = 0.1, 0.2, 0.3
    ta, tb, tc = K.turns(a), K.turns(b), K.turns(c)
    r = K.Rotator(a)
    r.schedule(150, b)      # beyond the first call: stays queued
    r.schedule(40, c)       # inside
    r.schedule(100, b)      # exactly at the end of the first call: for the next one
    assert rot_incs(r, 100) == [(0, 40, ta), (40, 60, tc)]
    assert r.counter == 100 and [o for o, _ in r.queue] == [100, 150]
    r.schedule(30, a)       # already behind the counter: dropped when reached
    assert rot_incs(r, 100) == [(0, 50, tb), (50, 50, tb)] and r.dropped == 1 and not r.queue
    # equal offsets: scheduling order, the last one wins, no sample sees the first
    r.schedule(250, a)
    r.schedule(250, c)
    assert rot_incs(r, 100) == [(0, 50, tb), (50, 50, tc)]
    # set_phase_inc acts at once and leaves the queue alone; the phase is continuous over all of it
    r2 = K.Rotator(a)
    r2.schedule(10, b)
    r2.set_phase_inc(c)
    assert rot_incs(r2, 20) == [(0, 10, tc), (10, 10, tb)]
    assert r2.phase == (10 * tc + 10 * tb) % K.ONE
    # seek == work without data; reset gives the constructor's state
    r3 = K.Rotator(a)
    r3.schedule(10, b)
    r3.seek(20)
    assert (r3.counter, r3.phase, r3.inc) == (20, (10 * ta + 10 * tb) % K.ONE, tb)
    r3.reset()
    assert (r3.counter, r3.phase, r3.inc, r3.queue) == (0, 0, ta, [])


def test_rotator_model_is_exact_far_out():
    # 2^40 samples of inc = 2 pi / 8 come back to phase 0 (up to the rounding of the double 2 pi / 8 itself, which the exact
    # model carries: (float(pi / 4) - pi / 4) 2^40 radians)
    inc = np.pi / 4
    r = K.Rotator(inc)
    r.seek(1 << 40)
    err_turns = (r.phase if r.phase < K.ONE // 2 else r.phase - K.ONE) / K.ONE
    assert abs(err_turns) < 2.0 ** -53 * (1 << 40) / 8
    x = np.ones(8, np.complex64)
    y, bound = r.work(x)
    assert np.abs(y - np.exp(1j * (M.PI2 * err_turns + inc * np.arange(8)))).max() < 1e-9
    assert bound.max() < 2e-6  # 2^40 samples out the bound is still of the order of float32 rounding


# ------------------------------------------------------------------ the guard over every input set of the GPU tests
def test_gpu_input_sets_stay_inside_their_caps():
    for name, seed, n, es, cap in K.RANDOM_SETS:
        for period in K.PERIODS:
            x, plscs = K.random_set(seed, n, es, period)
            for known in (False, True):  # SOF form (never corrected at these offsets) and the full form of a known-PLSC handle
                m = K.run(x, plscs, period, known)
                _, n_win, n_bad = K.comparable(m)
                print(f"{name} period {period} {'full' if known else 'sof'}: {n_win} windows, {n_bad} ineligible, "
                      f"largest bound {m['bound'].max():.2e}")
                assert n_bad <= cap * n_win, (name, period, known)
    assert set(np.concatenate([K.random_set(s, n, e, 1)[1] for _, s, n, e, _ in K.RANDOM_SETS])) == set(range(128))
    for x, plscs, period in (K.mode_switch_set() + (1,), K.streaming_set() + (4,)):
        m = K.run(x, plscs, period)
        assert K.comparable(m)[2] == 0
    for f in K.QA_OFFSETS + K.QA_CORRECTED:
        for full in (False, True):
            assert K.run(K.qa_unit_period(f), [K.QA_PLSC], 1, full)["eligible"].all()
            assert K.run(K.qa_period_two(f), [K.QA_PLSC] * 4, 2, full)["eligible"].all()


def test_end_to_end_point_leaves_a_residual_inside_the_fine_range():
    x, sofs, sent, plsc = K.e2e_stream()
    # the fixed-PLSC tracker reports exactly the transmitted frames at this offset (the timing metric is differential)
    import plsync_model as P
    met, _ = P.metric(x)
    recs, _, state, _ = P.track(met, P.make_decoder(x), 3, plsc)
    assert [r[0] for r in recs] == sofs and state == P.LOCKED and sent.shape[0] == len(sofs)
    p1, f, p2 = K.e2e_model(x, sofs, plsc)
    d1 = p1["bound"].max()
    print(f"pass 1 estimate {f:.6e} (true {K.E2E_FOFFSET}), bound {d1:.1e}; pass 2 estimates {np.abs(p2['foffset']).max():.2e} at most")
    assert p1["eligible"].all() and not p1["corrected"].any()
    # the true residual after the rotation, with the room a float32 estimate may take
    assert abs(K.E2E_FOFFSET - f) + d1 < K.RANGE
    # every frame's own second estimate is inside the range by twice both bounds: the device's f differs from the model's by
    # at most d1, which moves each second estimate by about as much, and its own float32 evaluation by at most its bound
    assert (K.RANGE - np.abs(p2["foffset"]) > 2 * (p2["bound"] + d1)).all() and p2["corrected"].all() and p2["eligible"].all()
