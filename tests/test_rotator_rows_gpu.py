"""GPU: the rotator rows (include/dvbs2_fec_hip.h, "rotator rows"; notes/rotator_rows.md) -- S rows rotated in one launch from records in
device memory, the retune and the frequency-control step.
  3. against the single-stream handle, bit for bit, over every access shape of the kernel;
  4. pieces, replay, and records that radians cannot express, against the Python-int model under the rotator's derived bound;
  5. retune equals Rotator.schedule;
  6. the control rule on synthetic arrays against the Python-int model, exactly, and every refusal;
  7. the stream contract of the three device entries;
  8. the frequency loop closes on three noisy carriers, without a host read in the control step.
The shapes are the smallest at which the code takes another path: 256 lanes and two samples per lane and step make 512 a tile, a row of
2^16 + 3 samples makes several tiles with a head and a tail, an odd stride alternates the 16-byte phase between rows."""
import functools

import numpy as np
import pytest

import fec_testlib as T
import loopback as L
import plframe_model as M
import rotator_rows_model as RM
import test_rotator_rows_host as H
from dvbs2rx_amd import (ROTATOR_STATE, Awgn, FecChain, PlCoarseBatch, PlFrontEnd, PlSync, PlSyncBatch, PulseShaper, Rotator, SymbolSync, awgn_sigma,
                         capi, pulse_geometry, rotator_control_device, rotator_retune_device, rotator_rows_device, rotator_state_init,
                         rotator_state_read)

pytestmark = pytest.mark.gpu
lib = capi.lib

INCS = (0.0123, -2.5, 1e-7, 3.0, -0.7)  # radians per sample, one per row
NMAX = (1 << 16) + 3
SIZES = (0, 1, 2, 3, 255, 256, 257, 511, 513, NMAX)
BASES = (0, 1, (1 << 31) + 1, 1 << 40)  # the last two make (m - index) * inc pass 2^64
STRIDES = ((0, 0), (1, 1), (6, 6), (1, 6), (6, 1))  # added to n: (in, out). n + 1 alternates the 16-byte phase of the rows; (1, 6) and (6, 1)
# put odd rows on the 8-byte path


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def dev_state(recs):
    """records on the device, 16-byte aligned"""
    t = dev(np.ascontiguousarray(recs).view(np.uint8))
    assert t.data_ptr() % 16 == 0
    return t


def host_state(t):
    return t.cpu().numpy().view(ROTATOR_STATE)


def bits(x):
    return np.ascontiguousarray(x, np.complex64).view(np.uint32).reshape(-1, 2)


@functools.lru_cache(None)
def samples():
    rng = np.random.default_rng(20260)
    x = (rng.normal(size=(len(INCS), NMAX)) + 1j * rng.normal(size=(len(INCS), NMAX))).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def single_reference(b):
    """per row the bits of Rotator(INCS[s]) after seek(b) over the row's NMAX samples; the bits of a shorter call are their prefix (a
    sample of the single handle does not depend on how its stream is cut into calls: tests/test_plcoarse_gpu.py)"""
    import torch
    out = []
    for s, inc in enumerate(INCS):
        rot = Rotator(inc)
        rot.seek(b)
        d = dev(samples()[s].view(np.float32))
        rot.work_device(d.data_ptr(), NMAX, d.data_ptr(), T.stream())
        torch.cuda.synchronize()
        out.append(d.cpu().numpy().view(np.uint32).reshape(-1, 2))
        rot.close()
    return out


def run_in_place(xs, n, stride, shift, call):
    """rows of n samples at shift + s * stride of a sentinel buffer, call(ptr, ptr), the rows back; everything else must be untouched"""
    import torch
    S = len(xs)
    total = shift + S * stride + T.PAD
    host = np.full((total, 2), T.SENTINEL, np.uint32)
    for s, x in enumerate(xs):
        host[shift + s * stride:shift + s * stride + n] = bits(x[:n])
    d = torch.from_numpy(host.view(np.int32)).cuda()
    assert d.data_ptr() % 16 == 0
    call(d.data_ptr() + 8 * shift, d.data_ptr() + 8 * shift)
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint32).reshape(-1, 2)
    touched = np.zeros(total, bool)
    for s in range(S):
        touched[shift + s * stride:shift + s * stride + n] = True
    assert (got[~touched] == T.SENTINEL).all(), "a write outside the rows"
    return [got[shift + s * stride:shift + s * stride + n] for s in range(S)]


# ------------------------------------------------------------------ 3. against the single-stream handle
@pytest.mark.parametrize("b", BASES)
def test_rows_equal_single_handles(b):
    """Row s with state_init(INCS[s]) and base_index = b equals Rotator(INCS[s]) after seek(b), bit for bit: S in {1, 2, 5}, every size,
    the strides n, n + 1 and n + 6 (and the two mixed), in and out at +0 / +8 bytes, in place and out of place. Everything around and
    between the rows stays the sentinel, the input is not written (T.run_strided)."""
    want = single_reference(b)
    x = samples()
    d_state = dev_state(rotator_state_init(INCS))
    n_calls = 0
    for S in (1, 2, 5):
        for n in SIZES:
            xs = [x[s, :n] for s in range(S)]
            for di, do in STRIDES:
                for in_shift in (0, 1):
                    for out_shift in (0, 1):
                        outs, _ = T.run_strided(lambda i, o: rotator_rows_device(i, n + di, o, n + do, n, S, b, d_state.data_ptr(), 0, T.stream()),
                                                xs, [n] * S, n + di, n + do, in_shift, out_shift)
                        for s in range(S):
                            T.same_bits(outs[s], want[s][:n], f"S {S}, n {n}, strides +{di} / +{do}, shifts {in_shift} / {out_shift}, row {s}")
                        n_calls += 1
                if di == do:
                    for shift in (0, 1):
                        outs = run_in_place(xs, n, n + di, shift, lambda i, o: rotator_rows_device(i, n + di, o, n + di, n, S, b, d_state.data_ptr(),
                                                                                                   0, T.stream()))
                        for s in range(S):
                            T.same_bits(outs[s], want[s][:n], f"in place: S {S}, n {n}, stride +{di}, shift {shift}, row {s}")
                        n_calls += 1
    assert n_calls == 3 * len(SIZES) * (5 * 4 + 3 * 2)
    assert host_state(d_state).tobytes() == rotator_state_init(INCS).tobytes(), "the rotation wrote a record"


# ------------------------------------------------------------------ 4. pieces, replay, records that radians cannot express
def random_states(rng):
    """six records: inc 0, 2^63, 2^64 - 1 and three random ones; random phases; an index in front of, inside and far behind the call,
    a negative one and one near 2^50"""
    u64 = lambda: int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))  # noqa: E731
    incs = [0, 1 << 63, (1 << 64) - 1, u64(), u64(), u64()]
    idx = [0, 5000, 1300, -12345, (1 << 50) + 7, 999]
    return [RM.state(u64(), inc, i, u64()) for inc, i in zip(incs, idx)]


def test_pieces_replay_and_model():
    """base_index 1000, 700 samples, records with index > base_index among them. One call == the same rows cut at 1, 255, 256, 257 with
    advancing base_index (the pieces start at other 16-byte phases than the whole) == the same call again, bit for bit; every sample
    within the derived bound of the float64 evaluation of the exact integer phase."""
    import torch
    rng = np.random.default_rng(4)
    states = random_states(rng)
    S, n, base, stride = len(states), 700, 1000, 701
    x = samples()[np.arange(S) % len(INCS), 100:100 + n] * np.arange(1, S + 1, dtype=np.float32)[:, None]
    d_state = dev_state(RM.to_records(states, ROTATOR_STATE))
    d_in = torch.zeros((S, stride, 2), dtype=torch.float32, device="cuda")
    d_in[:, :n] = dev(x.view(np.float32).reshape(S, n, 2))

    def call(d_out, a, k):
        rotator_rows_device(d_in.data_ptr() + 8 * a, stride, d_out.data_ptr() + 8 * a, stride, k, S, base + a, d_state.data_ptr(), 0, T.stream())

    outs = []
    for cuts in ([0, n], [0, n], [0, 1, 255, 256, 257, n]):
        d_out = T.sentinel(S * stride * 2)
        for a, e in zip(cuts[:-1], cuts[1:]):
            call(d_out, a, e - a)
        torch.cuda.synchronize()
        outs.append(d_out.cpu().numpy().view(np.uint32).reshape(S, stride, 2))
        assert (outs[-1][:, n:] == T.SENTINEL).all()
    assert np.array_equal(outs[0], outs[1]), "the same call twice gives other bits"
    assert np.array_equal(outs[0], outs[2]), "pieces differ from one call"
    got = np.ascontiguousarray(outs[0][:, :n]).view(np.complex64).reshape(S, n)
    for s, st in enumerate(states):
        exact, bound = RM.rotate(x[s], st, base)
        err = np.abs(got[s].astype(np.complex128) - exact)
        assert (err <= bound).all(), (s, float((err / bound).max()))
        assert err.max() > 0 or st["inc"] == 0  # (the comparison is not vacuous: float32 results differ from float64 ones)
    assert host_state(d_state).tobytes() == RM.to_records(states, ROTATOR_STATE).tobytes()


# ------------------------------------------------------------------ 5. retune equals schedule
def test_retune_equals_schedule():
    """Row 1 of three: blocks of 300 samples. A retune between two calls (at 300, the running count) and one in front of a block that
    spans it (at 457, inside the block 300..600: the caller cuts its call there) equal Rotator(inc).schedule(300, inc2).schedule(457,
    inc3) over the 600 samples, bit for bit. A call does not split itself: with the final record one call over 300..600 gives the
    scheduled bits from 457 on, and not in front of it. The record equals the model's integers; the other rows' records are untouched."""
    import torch
    inc, inc2, inc3, n = INCS[1], 0.31, -1.9, 600
    x = samples()[:3, :n]
    rot = Rotator(inc)
    rot.schedule(300, inc2)
    rot.schedule(457, inc3)
    want = bits(rot.work(np.ascontiguousarray(x[1])))
    rot.close()
    recs = rotator_state_init([INCS[0], inc, INCS[2]])
    recs["reserved"] = [11, 22, 33]
    d_state = dev_state(recs)
    d_in = dev(np.ascontiguousarray(x).view(np.float32))
    d_out = torch.zeros_like(d_in)
    st = T.stream()

    def rows(a, e):
        rotator_rows_device(d_in.data_ptr() + 8 * a, n, d_out.data_ptr() + 8 * a, n, e - a, 3, a, d_state.data_ptr(), 0, st)

    rows(0, 300)
    rotator_retune_device(d_state.data_ptr(), 1, 300, inc2, 0, st)
    rows(300, 457)
    rotator_retune_device(d_state.data_ptr(), 1, 457, inc3, 0, st)
    rows(457, n)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(3, n, 2)
    T.same_bits(got[1], want, "retunes at 300 and 457")
    model = RM.from_records(recs)
    RM.retune(model[1], 300, inc2)
    RM.retune(model[1], 457, inc3)
    after = host_state(d_state)
    assert after.tobytes() == RM.to_records(model, ROTATOR_STATE).tobytes(), (after, model)
    assert after[[0, 2]].tobytes() == recs[[0, 2]].tobytes() and int(after[1]["index"]) == 457 and int(after[1]["reserved"]) == 22
    for s in (0, 2):  # the other rows: one increment throughout
        one = Rotator(INCS[s])
        T.same_bits(got[s], bits(one.work(np.ascontiguousarray(x[s]))), f"row {s}")
        one.close()
    rows(300, n)
    torch.cuda.synchronize()
    again = d_out.cpu().numpy().view(np.uint32).reshape(3, n, 2)[1]
    T.same_bits(again[457:], want[457:], "one call over 300..600 with the final record, from 457 on")
    assert not np.array_equal(again[300:457], want[300:457])  # ... and the samples in front of 457 are NOT the scheduled ones


# ------------------------------------------------------------------ 6. the control rule
OFFSETS = [0, 0, 3, 4, 9, 9, 12]  # six streams: an empty one at the start and one in the middle
N_SLOTS = 12


def scenario(kind, n):
    """(coarse_foffset, coarse_corrected, new_est, fine_foffset, fine_valid) of a stream's n slots"""
    cf, cc, ne, ff, fv = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    if kind == "coarse":            # coarse only
        cf[:], ne[:] = np.linspace(0.02, 0.03, n), 1
    elif kind == "fine":            # fine only
        cc[:], ne[:], fv[:], ff[:], cf[:] = 1, 1, 1, np.linspace(-3e-4, -1e-4, n), 1e-4
    elif kind == "coarse-fine":     # coarse then fine: fine decides
        cf[:], ne[:] = 0.011, 1
        cc[n // 2:], fv[n // 2:], ff[n // 2:] = 1, 1, 2.5e-5
    elif kind == "fine-coarse":     # fine then an uncorrected new_est: coarse decides
        cc[:], fv[:], ff[:], ne[:] = 1, 1, 7e-5, 1
        cc[-1], fv[-1], cf[-1] = 0, 0, -0.04
    elif kind == "nothing":         # new_est with coarse_corrected = 1 and fine_valid = 0; fine values that must not be read as valid
        cc[:], ne[:], ff[:], cf[:] = 1, 1, 9e-5, 0.2
    elif kind == "nan":             # a qualifying NaN
        cf[:], ne[:] = np.nan, 1
    elif kind == "half":            # a qualifying estimate with |d| >= 0.5
        cf[:], ne[:] = 0.5, 1
    else:
        raise KeyError(kind)
    return cf, cc, ne, ff, fv


CONFIGS = {"a": ("coarse", "fine", "coarse-fine", "fine-coarse"), "b": ("nothing", "nan", "half", "coarse"),
           "c": ("fine-coarse", "half", "fine", "coarse-fine")}  # the kinds of streams 1, 2, 3 and 5


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_control_rule_equals_the_model(config):
    """inc, phase, index, d_applied and d_delta equal the Python-int model for max_slots 12, 10 (cuts the last stream) and 4, with and
    without the fine arrays, with and without d_applied / d_delta; a stream that is not steered keeps its 32 bytes, `reserved` stays."""
    import torch
    arrays = [np.zeros(N_SLOTS, t) for t in (np.float32, np.int32, np.int32, np.float32, np.int32)]
    for s, kind in zip((1, 2, 3, 5), CONFIGS[config]):
        a, b = OFFSETS[s], OFFSETS[s + 1]
        for dst, src in zip(arrays, scenario(kind, b - a)):
            dst[a:b] = src
    cf, cc, ne, ff, fv = arrays
    d = [dev(v) for v in arrays]
    d_off = dev(np.array(OFFSETS, np.int32))
    rng = np.random.default_rng(66)
    before = random_states(rng)
    at, cs, fs = 1 << 33, 1.0, 0.5  # (coarse scale 1: the estimate 0.5 does not apply)
    seen = set()
    for max_slots in (12, 10, 4):
        for fine in (True, False):
            for report in (True, False):
                states = [dict(st) for st in before]
                want_applied, want_delta = RM.control(OFFSETS, max_slots, cf, cc, ne, ff if fine else None, fv if fine else None, cs, fs, at, states)
                d_state = dev_state(RM.to_records(before, ROTATOR_STATE))
                d_applied = torch.full((6,), -7, dtype=torch.int32, device="cuda")
                d_delta = torch.full((6,), -7, dtype=torch.int64, device="cuda")
                rotator_control_device(d_off.data_ptr(), 6, max_slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr() if fine else 0,
                                       d[4].data_ptr() if fine else 0, cs, fs, at, d_state.data_ptr(), d_applied.data_ptr() if report else 0,
                                       d_delta.data_ptr() if report else 0, 0, T.stream())
                torch.cuda.synchronize()
                after = host_state(d_state)
                assert after.tobytes() == RM.to_records(states, ROTATOR_STATE).tobytes(), (config, max_slots, fine, report)
                assert d_applied.cpu().tolist() == (want_applied if report else [-7] * 6) and d_delta.cpu().tolist() == (want_delta if report else [-7] * 6)
                for s in range(6):
                    if want_applied[s] <= 0:
                        assert after[s].tobytes() == RM.to_records(before, ROTATOR_STATE)[s].tobytes()
                    else:
                        assert int(after[s]["index"]) == at and int(after[s]["reserved"]) == before[s]["reserved"]
                seen.update(want_applied)
                assert want_applied[0] == want_applied[4] == 0
    assert seen == {"a": {0, 1, 2}, "b": {-1, 0, 1}, "c": {-1, 0, 1, 2}}[config]


def test_control_and_retune_refusals_write_nothing():
    """every argument refusal of the three device entries with its exact text (the list of tests/test_rotator_rows_host.py, here on a
    machine that has a device), and the records behind a live pointer unchanged"""
    import torch
    recs = RM.to_records(random_states(np.random.default_rng(5)), ROTATOR_STATE)
    d_state = dev_state(recs)
    live = d_state.data_ptr()
    for changes, text in H.CONTROL_REFUSED:
        a = H.with_(H.with_(H.GOOD_CONTROL, _names=H.CONTROL_NAMES, d_state=live), _names=H.CONTROL_NAMES, **changes)
        T.refused(capi.EINVAL, text, lib.dvbs2_rotator_control_device, *[v or None if i in (0, 3, 4, 5, 6, 7, 11, 12, 13) else v for i, v in enumerate(a)], 0, None)
    for a, text in H.RETUNE_REFUSED:
        T.refused(capi.EINVAL, text, lib.dvbs2_rotator_retune_device, (live if a[0] == H.A else a[0]) or None, a[1], a[2], float(a[3]), 0, None)
    for changes, text in H.ROWS_REFUSED:
        a = H.with_(H.GOOD_ROWS, _names=H.ROWS_NAMES, **changes)
        T.refused(capi.EINVAL, text, lib.dvbs2_rotator_rows_device, *[v or None if i in (0, 2, 7) else v for i, v in enumerate(a)], 0, None)
    # a device that does not exist: refused behind the argument checks, by check_device
    T.refused(capi.EINVAL, "device index out of range", lib.dvbs2_rotator_retune_device, live, 0, 0, 0.1, 1 << 20, None)
    T.refused(capi.EINVAL, "device index out of range", lib.dvbs2_rotator_rows_device, live, 2, live, 2, 2, 1, 0, live, -1, None)
    T.refused(capi.EINVAL, "device index out of range", lib.dvbs2_rotator_control_device,
              *[live if i in (0, 3, 4, 5, 6, 7, 11) else None if i in (12, 13) else v for i, v in enumerate(H.GOOD_CONTROL)], 1 << 20, None)
    torch.cuda.synchronize()
    assert host_state(d_state).tobytes() == recs.tobytes()


# ------------------------------------------------------------------ 7. the stream contract
def contract_cases():
    """name -> (prepare() -> c, enqueue(c, stream), collect(c)): one device entry each, its input filled by a copy queued in front of it on
    the same stream"""
    import torch
    n, S = 5000, 3
    x = samples()[:S, :n]
    recs = RM.to_records(random_states(np.random.default_rng(8))[:S], ROTATOR_STATE)

    def prep_rows():
        return dict(src=dev(np.ascontiguousarray(x).view(np.float32).reshape(-1)), d_in=torch.zeros(S * n * 2, dtype=torch.float32, device="cuda"),
                    d_out=torch.zeros(S * n * 2, dtype=torch.float32, device="cuda"), src_state=dev_state(recs), d_state=dev_state(np.zeros(S, ROTATOR_STATE)))

    def rows(c, s):
        c["d_in"].copy_(c["src"], non_blocking=True)
        c["d_state"].copy_(c["src_state"], non_blocking=True)
        rotator_rows_device(c["d_in"].data_ptr(), n, c["d_out"].data_ptr(), n, n, S, 77, c["d_state"].data_ptr(), 0, s)

    def retune(c, s):
        c["d_state"].copy_(c["src_state"], non_blocking=True)
        rotator_retune_device(c["d_state"].data_ptr(), 2, 123456, -0.4, 0, s)
        rows_only(c, s)

    def rows_only(c, s):
        c["d_in"].copy_(c["src"], non_blocking=True)
        rotator_rows_device(c["d_in"].data_ptr(), n, c["d_out"].data_ptr(), n, n, S, 123456, c["d_state"].data_ptr(), 0, s)

    est = scenario("coarse", 1), scenario("fine", 1), scenario("coarse-fine", 2)
    arrays = [np.concatenate([e[k] for e in est]) for k in range(5)]

    def prep_control():
        c = prep_rows()
        c.update(src_est=[dev(a) for a in arrays], est=[torch.zeros(4, dtype=torch.float32 if a.dtype == np.float32 else torch.int32, device="cuda") for a in arrays],
                 off=dev(np.array([0, 1, 2, 4], np.int32)), applied=torch.zeros(S, dtype=torch.int32, device="cuda"),
                 delta=torch.zeros(S, dtype=torch.int64, device="cuda"))
        return c

    def control(c, s):
        c["d_state"].copy_(c["src_state"], non_blocking=True)
        for dst, src in zip(c["est"], c["src_est"]):
            dst.copy_(src, non_blocking=True)
        e = [t.data_ptr() for t in c["est"]]
        rotator_control_device(c["off"].data_ptr(), S, 4, e[0], e[1], e[2], e[3], e[4], 0.5, 0.5, 5000, c["d_state"].data_ptr(), c["applied"].data_ptr(),
                               c["delta"].data_ptr(), 0, s)
        rows_only(c, s)

    def collect(c):
        return {k: c[k].cpu().numpy().tobytes() for k in ("d_out", "d_state", "applied", "delta") if k in c}

    return {"rows": (prep_rows, rows, collect), "retune": (prep_rows, retune, collect), "control": (prep_control, control, collect)}


@pytest.mark.parametrize("name", ["rows", "retune", "control"])
def test_stream_contract(name):
    """The entry on a side stream while the null stream is held: it returns before the holds end (both streams are still pending behind
    the enqueue), is ordered behind the copies queued in front of it on its own stream (they fill its input and its records, behind a hold
    of that stream), and gives the bits of the serialized pass. The side stream's hold is sized as tests/test_stream_order_gpu.py sizes
    its own: 20 times the host time of the enqueues on a warm second serialized pass, and never below 100 ms here. Nothing is asserted about WHEN the
    side stream's work completes relative to the null stream's hold: whether two streams run side by side is the runtime's choice of
    hardware queue, not the entries' contract."""
    import gc
    import time

    import torch
    prepare, enqueue, collect = contract_cases()[name]
    want, host_ms = None, 0.0
    for _ in range(2):  # the first pass loads the code objects and is the expected value; the second must repeat it and is timed
        c = prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enqueue(c, 0)
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        got = collect(c)
        assert want is None or got == want, f"{name}: the serialized pass, repeated"
        want = got
    hold_ms = max(T.hold_for(host_ms), 100.0)  # (five times that file's floor: late in a long session the host has pauses of its own)
    print(f"rotator rows stream contract: {name}: host side of the enqueues {host_ms:.3f} ms, hold {hold_ms:.0f} ms")
    c = prepare()
    side, null = T.side_stream(), T.null_stream()
    torch.cuda.synchronize()
    gc.collect()  # now, so that no collection falls between the holds and the look at the streams
    T.hold(null, T.HOLD_MAX_MS)
    T.hold(side, hold_ms)
    with torch.cuda.stream(side):
        enqueue(c, side.cuda_stream)
    pending = T.pending(side), T.pending(null)
    side.synchronize()
    torch.cuda.synchronize()
    assert pending == (True, True), f"{name}: side / null stream pending behind the enqueue {pending}: the entry waited, or the hold of {hold_ms:.0f} ms was too short"
    got = collect(c)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], f"{name}: {k} behind a hold differs from the serialized pass"
    if name == "control":
        assert np.frombuffer(got["applied"], np.int32).tolist() == [1, 2, 2]


# ------------------------------------------------------------------ 8. the loop closes
PLSC, FRAME_LEN = L.PLSC, M.pls_parse(L.PLSC)["plframe_len"]
SLOT = FRAME_LEN + 90
F_TRUE = (0.02, -0.007, 1e-4)            # cycles per symbol: two far outside the fine range of 3.3875e-4, one inside it
LEADS, SEEDS = (400, 733, 150), (6101, 6102, 6103)
ES_N0_DB = 15.0                          # plcoarse_model.E2E_ES_N0_DB
FINE_RANGE = 3.3875e-4
# The block: three PLFRAMEs of samples per pass. With several frames per pass the LAST gathered frame of a pass lies whole in samples
# rotated by the pass's own increment, whatever the frame in front of it straddles; its estimate is the residual of that increment, so
# the loop gain is 1. Six passes: the first locks the tracker and gives the coarse step, the second the first fine step, two more for
# the fine steps to settle, and the last two are the ones whose every frame must decode.
BLOCK = 3 * FRAME_LEN * L.SPS
PASSES = 6
ND = 19                                  # PASSES * 3 frames and one more: the lead and the pending frame of the last pass
MAX_SLOTS = 16                           # at most four frames per stream and pass, and room to spare
SYM_CAP = 1 << 16


@functools.lru_cache(None)
def carriers():
    """(sent [3][ND, in_bytes], the samples on the device float32 [3, ns, 2], ns): per carrier ND short QPSK 1/4 frames with pilots,
    shaped at L.SPS with unit_amplitude_taps, moved by its offset with a Rotator, noise at Es/N0 15 dB from an Awgn with fixed seeds"""
    import torch
    st = T.stream()
    history = pulse_geometry(L.SPS, L.RRC_DELAY)[1]
    sent, ys = [], []
    for c, (f, lead, seed) in enumerate(zip(F_TRUE, LEADS, SEEDS)):
        sent_c, d_x, n, n_all, _ = L.transmit_symbols([PLSC] * ND, ND, L.GOLD, lead, seed, flush=history + 64)
        ps = PulseShaper(L.SPS, taps=L.unit_amplitude_taps(L.SPS, L.ROLLOFF, L.RRC_DELAY, L.TAU), max_symbols=n_all)
        ns = n_all * L.SPS
        d_y = torch.zeros((ns, 2), dtype=torch.float32, device="cuda")
        ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), ns, st)
        power = float((d_y[:n * L.SPS] ** 2).sum(dim=1).mean().item())
        rot = Rotator(2.0 * np.pi * f / L.SPS)
        rot.work_device(d_y.data_ptr(), ns, d_y.data_ptr(), st)
        noise = Awgn(seed=900 + c, sigma=awgn_sigma(ES_N0_DB, es=power, sps=L.SPS), max_samples=ns)
        noise.work_device(d_y.data_ptr(), ns, ns, 1, d_y.data_ptr(), ns, first_stream=c, first_index=0, stream=st)
        torch.cuda.synchronize()
        for o in (noise, rot, ps):
            o.close()
        sent.append(sent_c)
        ys.append(d_y)
    ns = min(int(y.shape[0]) for y in ys)
    assert ns >= PASSES * BLOCK
    return sent, torch.stack([y[:ns] for y in ys]).contiguous(), ns


def run_loop(scale):
    """PASSES passes over blocks of BLOCK samples of the three carriers, the control step with both scales `scale`. Returns dict(applied
    [PASSES, 3], inc: the records' increments behind every pass in cycles per sample [PASSES, 3], state: the final records, frames: per
    pass the list of (stream, encoder frame, message bytes or None) of every gathered slot -- decoded for the last two passes only)."""
    import torch
    st = T.stream()
    S = 3
    sent, d_y, ns = carriers()
    ss = SymbolSync(sps=L.SPS, loop_bw=0.01, damping=1.0, rolloff=L.ROLLOFF, interp_method=0, max_streams=S, max_samples=BLOCK + 64)
    # the tracker in its known-PLSC mode (the reference's "PLSC decoder disabled", as tests/test_plcoarse_gpu.py's end-to-end point): the
    # coherent PLSC decode does not survive 0.02 cycles per symbol, and the open-loop de-rotation the reference puts in front of it is not
    # restated (include/dvbs2_fec_hip.h under dvbs2_plcoarse_*)
    ps = PlSyncBatch(plsc=PLSC, max_streams=S, max_symbols=SYM_CAP, max_frames=16)
    pcb = PlCoarseBatch(1, PLSC, max_streams=S, max_slots=MAX_SLOTS)
    fe = PlFrontEnd(L.GOLD, PLSC, max_frames=MAX_SLOTS)
    xl = fe.xfecframe_len
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    d_state = dev_state(rotator_state_init([0.0] * S))
    d_new, d_smp, d_tmp, d_sym = z(S, BLOCK, 2), z(S, BLOCK + 64, 2), z(S, BLOCK, 2), z(S, SYM_CAP, 2)
    d_slots, d_fo, d_cc, d_ne = z(MAX_SLOTS * SLOT * 2), z(MAX_SLOTS), z(MAX_SLOTS, dtype=torch.int32), z(MAX_SLOTS, dtype=torch.int32)
    d_ff, d_fv = z(MAX_SLOTS), z(MAX_SLOTS, dtype=torch.int32)
    d_applied, d_hist = z(PASSES, S, dtype=torch.int32), z(PASSES, S * 32, dtype=torch.uint8)
    d_rec = [z(S * 16 * 16, dtype=torch.uint8) for _ in range(PASSES)]
    d_off, d_sr = [z(S + 1, dtype=torch.int32) for _ in range(PASSES)], [z(2 * MAX_SLOTS, dtype=torch.int32) for _ in range(PASSES)]
    d_rx = [z(MAX_SLOTS, xl * 2) for _ in range(PASSES)]
    left_smp, left_sym = [0] * S, [0] * S
    for p in range(PASSES):
        count = p * BLOCK  # the ONE running sample count: base_index of this pass, at_index of the last pass's control step
        rotator_rows_device(d_y.data_ptr() + 8 * count, ns, d_new.data_ptr(), BLOCK, BLOCK, S, count, d_state.data_ptr(), 0, st)
        for s in range(S):  # torch plumbing: the new samples behind what the timing loop left unconsumed
            d_smp[s, left_smp[s]:left_smp[s] + BLOCK] = d_new[s]
        n_in = [left_smp[s] + BLOCK for s in range(S)]
        ss.work_device(d_smp.data_ptr(), BLOCK + 64, n_in, d_tmp.data_ptr(), BLOCK, BLOCK, 0, 0, st)
        n_out, used, status = ss.finish()  # a host read the stage needs: the symbol counts are host arguments of the search
        assert status.tolist() == [0] * S
        for s in range(S):
            left_smp[s] = n_in[s] - int(used[s])
            assert 0 <= left_smp[s] <= 64
            d_smp[s, :left_smp[s]] = d_smp[s, int(used[s]):n_in[s]].clone()
            d_sym[s, left_sym[s]:left_sym[s] + int(n_out[s])] = d_tmp[s, :int(n_out[s])]
        n_sym = [left_sym[s] + int(n_out[s]) for s in range(S)]
        assert max(n_sym) <= SYM_CAP
        ps.work_device(d_sym.data_ptr(), SYM_CAP, [0] * S, n_sym, d_rec[p].data_ptr(), st)
        ps.gather_device(d_sym.data_ptr(), SYM_CAP, d_rec[p].data_ptr(), S, PLSC, d_slots.data_ptr(), MAX_SLOTS, d_off[p].data_ptr(), d_sr[p].data_ptr(), st)
        pcb.work_device(d_slots.data_ptr(), SLOT, d_off[p].data_ptr(), S, 0, d_fo.data_ptr(), d_cc.data_ptr(), d_ne.data_ptr(), st)
        # (the frame count of the launch is a host argument: all slots, so that no count is read back; the control step and the checks
        # below look at the slots below d_offsets[S] only)
        fe.work_strided_device(d_slots.data_ptr(), SLOT, MAX_SLOTS, d_cc.data_ptr(), d_fo.data_ptr(), d_rx[p].data_ptr(), st,
                               fine_foffset=d_ff.data_ptr(), fine_valid=d_fv.data_ptr())
        rotator_control_device(d_off[p].data_ptr(), S, MAX_SLOTS, d_fo.data_ptr(), d_cc.data_ptr(), d_ne.data_ptr(), d_ff.data_ptr(), d_fv.data_ptr(),
                               scale, scale, count + BLOCK, d_state.data_ptr(), d_applied[p].data_ptr(), 0, 0, st)
        d_hist[p].copy_(d_state, non_blocking=True)
        _, consumed, _ = ps.finish()  # the other host read: where every stream is presented from next
        for s in range(S):
            left_sym[s] = n_sym[s] - int(consumed[s])
            d_sym[s, :left_sym[s]] = d_sym[s, int(consumed[s]):n_sym[s]].clone()
    torch.cuda.synchronize()
    hist = d_hist.cpu().numpy().view(ROTATOR_STATE).reshape(PASSES, S)
    inc = np.where(hist["inc"] >= 1 << 63, hist["inc"].astype(np.float64) - 2.0 ** 64, hist["inc"].astype(np.float64)) / 2.0 ** 64
    chain = FecChain(group_size=4, max_frames=MAX_SLOTS, max_trials=25, **L.QPSK_1_4_SHORT)
    chain.set_descramble(True)
    frames = []
    for p in range(PASSES):
        off, sr = d_off[p].cpu().numpy(), d_sr[p].cpu().numpy().reshape(MAX_SLOTS, 2)
        recs = d_rec[p].cpu().numpy().view(PlSync.FRAME_DTYPE).reshape(S, 16)
        total = int(off[S])
        assert total <= MAX_SLOTS
        msg = None
        if p >= PASSES - 2 and total:  # ONE FecChain call over all gathered frames of the pass
            msg, _, _ = chain.work(d_rx[p].cpu().numpy().view(np.complex64).reshape(MAX_SLOTS, xl)[:total], np.float32(10.0 ** (-ES_N0_DB / 10.0)))
        got = []
        for i in range(total):
            s, f = int(sr[i, 0]), int(sr[i, 1])
            assert off[s] <= i < off[s + 1]
            k = int(round((int(recs[s, f]["sof_index"]) - LEADS[s]) / FRAME_LEN))
            assert 0 <= k < ND and abs(int(recs[s, f]["sof_index"]) - LEADS[s] - k * FRAME_LEN) <= 24
            got.append((s, k, None if msg is None else msg[i].tobytes()))
        frames.append(got)
    for o in (chain, fe, pcb, ps, ss):
        o.close()
    return dict(applied=d_applied.cpu().numpy(), inc=inc, state=host_state(d_state), frames=frames, sent=sent)


def test_the_frequency_loop_closes():
    """Three carriers at +0.02, -0.007 and +1e-4 cycles per symbol behind noise at 15 dB. Per pass: rotator rows -> SymbolSync -> PlSyncBatch
    search and gather -> PlCoarseBatch -> strided front end -> rotator_control_device, which reads nothing back. Every stream's final
    increment is within 3.3875e-4 / sps cycles per sample of minus its offset; the far streams take a coarse step first and fine steps
    later, the third none but fine ones; every frame gathered in the last two passes decodes. With both scales 0 no frame of the far
    streams decodes and every frame of the third still does."""
    r = run_loop(1.0 / L.SPS)
    want = -np.array(F_TRUE) / L.SPS
    for p in range(PASSES):
        print(f"rotator rows loop: pass {p + 1}: applied {r['applied'][p].tolist()}, residual in cycles per symbol "
              + ", ".join(f"{v:+.3e}" for v in (r["inc"][p] - want) * L.SPS) + f", frames gathered {[sum(1 for f in r['frames'][p] if f[0] == s) for s in range(3)]}")
    final = rotator_state_read(r["state"])[0] / (2.0 * np.pi)
    assert (np.abs(final - want) <= FINE_RANGE / L.SPS).all(), (final - want) * L.SPS
    assert np.allclose(final, r["inc"][-1], rtol=0, atol=1e-15)
    for s in (0, 1):
        steps = [int(a) for a in r["applied"][:, s] if a != 0]
        n_coarse = steps.count(1)
        assert steps[0] == 1 and steps == [1] * n_coarse + [2] * (len(steps) - n_coarse) and len(steps) - n_coarse >= 3, (s, steps)
    assert set(r["applied"][:, 2].tolist()) <= {0, 2} and 2 in r["applied"][:, 2].tolist(), r["applied"][:, 2]
    for p in (PASSES - 2, PASSES - 1):
        assert [sum(1 for f in r["frames"][p] if f[0] == s) >= 2 for s in range(3)] == [True] * 3  # several frames per stream and pass
        for s, k, msg in r["frames"][p]:
            assert msg == r["sent"][s][k].tobytes(), f"pass {p + 1}: stream {s}, encoder frame {k}"
    z = run_loop(0.0)
    assert not z["inc"].any() and set(z["applied"][:, :2].ravel().tolist()) <= {0, 1}
    for p in (PASSES - 2, PASSES - 1):
        ok = [(s, msg == z["sent"][s][k].tobytes()) for s, k, msg in z["frames"][p]]
        assert not any(good for s, good in ok if s < 2), f"open loop, pass {p + 1}: a frame of a far stream decoded: {ok}"
        assert all(good for s, good in ok if s == 2) and sum(1 for s, _ in ok if s == 2) >= 2, f"open loop, pass {p + 1}: {ok}"
