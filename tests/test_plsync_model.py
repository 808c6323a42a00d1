"""CPU tests of the PLFRAME search: the host-only entries of the library against the float64 model of plsync_model.py, the
model against the reference's own unit-test scenarios (lib/qa_pl_frame_sync.cc:191-416), and the guard that vouches for
every seeded stream the GPU tests run: no decision of the model's tracker lies within float32 rounding of a threshold or a
tie, so the device has to reproduce every record exactly and no stream needs to be excused."""
import numpy as np
import pytest

import plframe_model as M
import plsync_model as P


# ------------------------------------------------------------------ the library's host-only entries
def test_library_exports_the_plsync_entries():
    from dvbs2rx_amd import capi
    for name in ("create", "destroy", "reset", "set_plsc_mode", "set_expected_pls", "metric_device", "search_device", "finish",
                 "search", "gather_device", "taps", "thresholds"):
        assert hasattr(capi.lib, "dvbs2_plsync_" + name), name
        assert "dvbs2_plsync_" + name in capi.SYMBOLS


def test_taps_and_thresholds_equal_the_model():
    import dvbs2rx_amd
    sof, pl = dvbs2rx_amd.plsync_taps()
    assert sof.tolist() == P.SOF_TAPS.tolist() and pl.tolist() == P.PLSC_TAPS.tolist()
    assert set(np.abs(sof)) == {1.0} and set(np.abs(pl)) == {1.0}
    assert dvbs2rx_amd.plsync_thresholds() == (P.THRESHOLD_U, P.THRESHOLD_L) == (30.0, 25.0)
    # the library's expected symbols give the same differentials as the model's
    h = dvbs2rx_amd.plheader_symbols(0).astype(np.complex128)
    tap = h[1:] * np.conj(h[:-1])
    assert np.array_equal(np.sign(tap.imag[0:25]), P.SOF_TAPS) and np.array_equal(np.sign(tap.imag[26:89:2]), P.PLSC_TAPS)


def test_frame_record_layout():
    import ctypes as C
    from dvbs2rx_amd import PlSync, capi
    assert PlSync.FRAME_DTYPE.itemsize == C.sizeof(capi.PlSyncFrame) == 16
    for f in ("sof_index", "metric", "plsc", "flags"):
        assert PlSync.FRAME_DTYPE.fields[f][1] == getattr(capi.PlSyncFrame, f).offset


# ------------------------------------------------------------------ the model itself
def test_bit0_flips_the_plsc_taps_and_nothing_else_changes_them():
    for p in range(128):
        h = M.plheader(p)
        tap = np.round((h[1:] * np.conj(h[:-1])).imag)
        assert np.array_equal(tap[0:25], P.SOF_TAPS)
        assert np.array_equal(tap[26:89:2], -P.PLSC_TAPS if p & 1 else P.PLSC_TAPS), p


def test_clean_header_of_every_plsc_peaks_at_57_on_its_last_symbol():
    worst = 0.0
    for p in range(128):
        rng = np.random.default_rng(p)
        x = np.concatenate([P.qpsk(rng, 200), M.plheader(p), P.qpsk(rng, 200)]).astype(np.complex64)
        m, bound = P.metric(x)
        assert abs(m[289] - 57.0) <= bound[289] + 1e-5  # the symbols are float32: 57 up to their own rounding
        off = np.delete(m, 289)
        worst = max(worst, off.max())
        assert (off <= P.THRESHOLD_U).all(), p
    print(f"peak 57.00 for all 128 PLSCs, largest off-peak value {worst:.2f}")


def test_metric_history_equals_one_long_buffer():
    rng = np.random.default_rng(3)
    x = np.concatenate([P.qpsk(rng, 150), M.plheader(77), P.qpsk(rng, 150)]).astype(np.complex64)
    whole, _ = P.metric(x)
    for cut in (1, 89, 200, 239, 240, 300):
        hist = np.concatenate([np.zeros(P.HIST, np.complex64), x[:cut]])[-P.HIST:]
        part, _ = P.metric(x[cut:], hist)
        assert np.allclose(part, whole[cut:], rtol=0, atol=1e-12)


def qa_stream(parts):
    return np.concatenate(parts).astype(np.complex64)


QA_PLSC = P.plsc_of(4, 1, 1)


def qa_parts():
    info = M.pls_parse(QA_PLSC)
    n = info["payload_len"]
    payload = np.exp(1j * M.PI2 * np.arange(n) / n)
    return info, M.plheader(QA_PLSC), payload, np.full(90, 1j)


def states_after(x, lens, unlock_thresh):
    """step the model over x symbol by symbol, as the reference's tests do; lens: {index: frame length told after that index}"""
    met, _ = P.metric(x)
    fs = P.FrameSync(unlock_thresh)
    states, sofs = [], []
    for n, m in enumerate(met):
        is_sof, _ = fs.step(m)
        if is_sof:
            sofs.append(n)
        if n in lens:
            fs.frame_len = lens[n]
        states.append(fs.state)
    return states, sofs


def test_qa_locking_unlocking_threshold_1():  # lib/qa_pl_frame_sync.cc:191-256
    info, hdr, pay, junk = qa_parts()
    L = info["plframe_len"]
    st, sofs = states_after(qa_stream([hdr, pay, hdr, pay, junk]), {89: L}, 1)
    assert st[89] == P.FOUND and st[L - 1] == P.FOUND and st[L + 89] == P.LOCKED and st[2 * L - 1] == P.LOCKED
    assert st[2 * L + 89] == P.SEARCHING and sofs == [89, L + 89]


def test_qa_consecutive_sofs_after_wrong_frame_len():  # :258-296
    info, hdr, pay, _ = qa_parts()
    L = info["plframe_len"]
    st, sofs = states_after(qa_stream([hdr, np.ones(L - 90), hdr]), {89: 100}, 1)
    assert st[89] == P.FOUND and st[L - 1] == P.FOUND and st[L + 89] == P.FOUND and sofs == [89, L + 89]


def test_qa_sof_after_wrong_frame_len_while_locked():  # :298-336
    info, hdr, pay, _ = qa_parts()
    L = info["plframe_len"]
    st, sofs = states_after(qa_stream([hdr, np.ones(L - 90), hdr, np.ones(L - 90)]), {89: L, L + 89: 100}, 1)
    assert st[L + 89] == P.LOCKED and st[L + 89 + 99] == P.LOCKED and st[L + 89 + 100] == P.SEARCHING and st[-1] == P.SEARCHING
    assert sofs == [89, L + 89]


def test_qa_unlock_threshold_2():  # :354-416
    info, hdr, pay, _ = qa_parts()
    L = info["plframe_len"]
    rng = np.random.default_rng(5)

    def noisy():
        h = hdr + np.sqrt(10.0 / 2) * (rng.normal(size=90) + 1j * rng.normal(size=90))  # Es/N0 -10 dB
        return h / np.sqrt(np.mean(np.abs(h) ** 2))
    x = qa_stream([hdr, np.ones(L - 90), hdr, np.ones(L - 90), noisy(), np.ones(L - 90), noisy()])
    met, _ = P.metric(x)
    assert met[2 * L + 89] < P.THRESHOLD_L and met[3 * L + 89] < P.THRESHOLD_L
    st, sofs = states_after(x, {89: L}, 2)
    assert st[L + 89] == P.LOCKED and st[2 * L + 89] == P.LOCKED and st[3 * L + 88] == P.LOCKED and st[3 * L + 89] == P.SEARCHING
    assert sofs == [89, L + 89, 2 * L + 89]  # the first miss is an inferred peak (:242), the second unlocks


def test_track_equals_symbol_by_symbol_stepping():
    name, stream, trk = next(c for c in P.cases() if c[0] == "removed-2")
    c = P.build_case(name, stream, trk)
    dec = P.make_decoder(c["x"])
    fs, recs = P.FrameSync(2), []
    for n, m in enumerate(c["met"]):
        is_sof, is_peak = fs.step(m)
        if is_sof:
            plsc = dec(n)
            recs.append((n - 89, float(m), plsc, (1 if is_peak else 0) | (2 if fs.state == P.LOCKED else 0)))
            fs.frame_len = M.pls_parse(plsc)["plframe_len"]
    assert recs[:len(c["recs"])] == c["recs"] and len(recs) - len(c["recs"]) <= 1  # the last header may lack its frame


# ------------------------------------------------------------------ the guard over every stream of the GPU tests
@pytest.mark.parametrize("name,stream,trk", P.all_cases(), ids=[c[0] for c in P.all_cases()])
def test_guard_no_stream_is_excused(name, stream, trk):
    c = P.build_case(name, stream, trk)
    near, unclear = P.guard(c)
    visited = sum(v[2] - v[1] if v[0] == "u" else 1 for v in c["visits"])
    print(f"{name}: {c['x'].size} symbols, {visited} metrics compared, {len(c['recs'])} records, {len(c['log'])} decodes, "
          f"{near} near a threshold, {unclear} unclear decisions")
    assert near == 0 and unclear == 0


def test_streams_exercise_what_they_are_meant_to():
    by = {c[0]: P.build_case(*c) for c in P.cases() if c[0].startswith(("removed", "acm-11", "ccm-16-0-fixed", "ccm-16-clean-decode"))}
    assert [r[2] for r in by["acm-11"]["recs"]] == P.ACM_PLSCS and by["acm-11"]["state"] == P.LOCKED
    assert [r[0] for r in by["ccm-16-clean-decode"]["recs"]] == by["ccm-16-clean-decode"]["sofs"]
    assert len(by["ccm-16-0-fixed"]["recs"]) > 1000  # false detections in plenty at 0 dB
    inferred = {k: sum(1 for r in v["recs"] if not r[3] & 1) for k, v in by.items()}
    assert inferred["removed-1"] == 0 and inferred["removed-2"] == 1 and inferred["removed-3"] == 2
    assert all(by[f"removed-{u}"]["state"] == P.LOCKED for u in (1, 2, 3))  # each of them locks again
