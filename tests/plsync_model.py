"""float64 model of the PLFRAME search (dvbs2_plsync_*), written from the reference's text (lib/pl_frame_sync.cc,
lib/pl_frame_sync.h, lib/plsync_cc_impl.cc) on top of plframe_model.py. The taps are derived from the expected PLHEADER
symbols of PLSC 0, the metric is the clean sliding correlation (see include/dvbs2_fec_hip.h for the one defined
difference from the reference's even / odd delay lines), and the state machine is restated step by step with line
numbers. Also the seeded streams the GPU tests use, so that the CPU guard test can vouch for every one of them."""
import numpy as np

import plframe_model as M

THRESHOLD_U, THRESHOLD_L = 30.0, 25.0  # lib/pl_frame_sync.h:160-162
SEARCHING, FOUND, LOCKED = 0, 1, 2
HIST = 89
REAL_PEAK, FLAG_LOCKED = 1, 2


def derive_taps():
    """Imaginary parts of the +-j taps in header order: 25 SOF taps (positions 1..25), 32 PLSC taps (27, 29 .. 89). The tap
    is the conjugate of the expected differential conj(h_k) h_{k-1} (matched filter, lib/pl_frame_sync.cc:37-52, :99)."""
    h = M.plheader(0)
    e = np.conj(h[1:]) * h[:-1]  # e[k - 1]: expected differential at header position k
    tap = np.conj(e)
    assert np.allclose(tap.real, 0.0, atol=1e-12) and np.allclose(np.abs(tap.imag), 1.0, atol=1e-12)
    t = np.round(tap.imag)
    return t[0:25].copy(), t[26:89:2].copy()


SOF_TAPS, PLSC_TAPS = derive_taps()
SOF_POS = np.arange(1, 26)
PLSC_POS = np.arange(27, 90, 2)


def metric(x, history=None):
    """metric[n] = max(|S + P|, |S - P|) for every index of x, with the 89 symbols before x[0] in `history` (zeros when None),
    and the bound of a float32 evaluation: every differential is two products and a sum (3 roundings, <= 3 u |x_k| |x_{k-1}|
    as a complex error, u = 2^-24), the 57 terms are summed to a depth of at most 34 (<= 49 u sum |d_k|), the two squared
    moduli and the root add 3 u: 55 u sum |d_k| in all. The bound used is 65 * 2^-23 = 130 u, a factor above 2 in hand.
    plframe_model.sum_and_bound is not reused for it: that function bounds the ANGLE of a sum (it divides by |sum| and adds
    atan2f's error), while the thresholds compare the MODULUS; its summation term alone, 4 L 2^-24 sum |term| with L = 57, would
    be 228 u sum |d_k|, looser than the bound derived here."""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    hist = np.zeros(HIST, np.complex128) if history is None else np.asarray(history, np.complex64).astype(np.complex128)
    assert hist.shape == (HIST,)
    xx = np.concatenate([hist, x])
    d = np.zeros(xx.size, np.complex128)
    d[1:] = np.conj(xx[1:]) * xx[:-1]        # d[i]: differential of xx[i]; output n looks at xx[n + k], k = header position
    a = np.zeros(xx.size)
    a[1:] = np.abs(xx[1:]) * np.abs(xx[:-1])
    n = x.size
    S, P, mass = np.zeros(n, np.complex128), np.zeros(n, np.complex128), np.zeros(n)
    for k, t in zip(SOF_POS, SOF_TAPS):
        S += d[k:k + n] * (1j * t)
        mass += a[k:k + n]
    for k, t in zip(PLSC_POS, PLSC_TAPS):
        P += d[k:k + n] * (1j * t)
        mass += a[k:k + n]
    return np.maximum(np.abs(S + P), np.abs(S - P)), 65.0 * 2.0 ** -23 * mass + 1e-30


class FrameSync:
    """frame_sync::step (lib/pl_frame_sync.cc:66-243) as a function of the timing metric of the current symbol."""

    def __init__(self, unlock_thresh=3, frame_len=0):
        self.unlock_thresh, self.state, self.frame_len, self.sym_cnt, self.unlock_cnt = unlock_thresh, SEARCHING, frame_len, 0, 0

    def skippable(self):
        """how many coming symbols cannot change anything but the count: locked and before the expected index (:89-92, :127-128)"""
        return max(self.frame_len - self.sym_cnt - 1, 0) if self.state == LOCKED else 0

    def step(self, m):
        self.sym_cnt += 1                                                    # :68
        locked = self.state == LOCKED
        if locked and self.sym_cnt < self.frame_len:                         # :89-92, :127-128
            return False, False
        is_peak = m > THRESHOLD_L if locked else m > THRESHOLD_U             # :168-169
        peak_expected = locked                                               # :175
        if is_peak:                                                          # :183-193
            if self.state == SEARCHING:
                self.state = FOUND
            elif self.state == FOUND and self.sym_cnt == self.frame_len:
                self.state = LOCKED
            self.unlock_cnt = 0
        elif peak_expected:                                                  # :201-217
            self.unlock_cnt += 1
            if self.unlock_cnt == self.unlock_thresh:
                self.state = SEARCHING
                self.unlock_cnt = 0
        if is_peak or peak_expected:                                         # :220-230
            self.sym_cnt = 0
        return (is_peak or peak_expected) and self.state != SEARCHING, is_peak  # :242


def track(met, decode, unlock_thresh=3, fixed_plsc=-1, max_frames=None, frame_len_of=None):
    """The tracker over the metric of ONE buffer starting at reset. decode(n) gives the PLSC of the 90 symbols ending at n
    (lib/plsync_cc_impl.cc:880, :582-594); fixed_plsc >= 0 skips it (:145-159). A header is reported while its whole frame and
    the 90 symbols after it lie inside the buffer and fewer than max_frames records are written; the first one that is not
    ends the call. Returns (records [(sof_index, metric, plsc, flags)], consumed, state, visits): visits lists what was
    compared with which threshold, ('u', a, b) = every index of [a, b) with 30, ('l', n) = index n with 25."""
    met = np.asarray(met)
    n_syms = met.size
    length = frame_len_of or (lambda p: M.pls_parse(p)["plframe_len"])
    fs = FrameSync(unlock_thresh, length(fixed_plsc) if fixed_plsc >= 0 else 0)
    above = np.flatnonzero(met > THRESHOLD_U)
    recs, visits, n = [], [], 0
    while n < n_syms:
        if fs.state == LOCKED:
            skip = fs.skippable()
            if n + skip >= n_syms:
                break
            fs.sym_cnt += skip
            n += skip
            visits.append(("l", n))
        else:  # every index up to the next one above 30 is stepped and does nothing but count
            j = np.searchsorted(above, n)
            nxt = int(above[j]) if j < above.size else n_syms
            visits.append(("u", n, min(nxt + 1, n_syms)))
            fs.sym_cnt += nxt - n
            n = nxt
            if n >= n_syms:
                break
        before = (fs.state, fs.sym_cnt, fs.unlock_cnt)
        is_sof, is_peak = fs.step(met[n])
        if is_sof:
            plsc = fixed_plsc if fixed_plsc >= 0 else int(decode(n))
            new_len = length(plsc)
            if (max_frames is not None and len(recs) >= max_frames) or n - 89 + new_len + 90 > n_syms:
                fs.state, fs.sym_cnt, fs.unlock_cnt = before
                return recs, max(n - 89, 0), fs.state, visits
            recs.append((n - 89, float(met[n]), plsc, (REAL_PEAK if is_peak else 0) | (FLAG_LOCKED if fs.state == LOCKED else 0)))
            fs.frame_len = new_len                                            # set_frame_len, lib/plsync_cc_impl.cc:594
        n += 1
    return recs, n_syms, fs.state, visits


def header_at(x, n):
    """the 90 symbols ending at index n, zeros before the stream"""
    xx = np.concatenate([np.zeros(HIST, np.complex64), np.asarray(x, np.complex64)])
    return xx[n:n + 90]


def make_decoder(x, coherent=True, soft=True, enabled=None, log=None):
    """decode(n) for track(); log (a list) receives (n, clear) per call: clear = the decision is outside float32 rounding (soft:
    the two best metrics more than soft_tau apart; hard: every decision variable eligible)."""
    def decode(n):
        h = header_at(x, n)[None, :]
        if log is not None:
            if coherent and soft:
                m = np.sort(M.soft_metrics(h, enabled)[0])
                log.append((n, bool(m[-1] - m[-2] > M.soft_tau(h)[0])))
            else:
                log.append((n, bool(M.hard_eligible(h, coherent)[0])))
        return int(M.plsc_decode(h, coherent, soft, enabled)[0])
    return decode


# ------------------------------------------------------------------ seeded streams of the GPU tests
def plsc_of(modcod, short, pilots):
    return (modcod << 2) | (short << 1) | pilots


def qpsk(rng, n):
    return ((1 - 2.0 * rng.integers(0, 2, n)) + 1j * (1 - 2.0 * rng.integers(0, 2, n))) * M.S


def make_stream(plscs, seed, es_n0_db=None, offset=None, gold=0, removed=(), tail=300, phase=None, foffset=0.0, data=None):
    """`offset` random QPSK symbols, the PLFRAMEs of `plscs` back to back (headers of the frames listed in `removed` replaced by
    random QPSK), a closing PLHEADER of the last PLSC and `tail` random symbols; one phasor over the whole stream, then AWGN.
    Returns (stream complex64, list of true SOF indices, offset)."""
    rng = np.random.default_rng(seed)
    offset = int(rng.integers(0, 3000)) if offset is None else offset
    parts, sofs, pos = [qpsk(rng, offset)], [], offset
    for i, p in enumerate(plscs):
        f, _ = M.make_plframes(p, gold, 1, rng, data=None if data is None else data[i][None, :])
        f = f.reshape(-1).astype(np.complex128)
        if i in removed:
            f[:90] = qpsk(rng, 90)
        parts.append(f)
        sofs.append(pos)
        pos += f.size
    parts += [M.plheader(plscs[-1]), qpsk(rng, tail)]
    tx = np.concatenate(parts)
    ph = rng.uniform(-np.pi, np.pi) if phase is None else phase
    rx = tx * np.exp(1j * (ph + M.PI2 * foffset * np.arange(tx.size)))
    if es_n0_db is not None:
        n0 = 10.0 ** (-es_n0_db / 10.0)
        rx = rx + np.sqrt(n0 / 2.0) * (rng.normal(size=rx.size) + 1j * rng.normal(size=rx.size))
    return rx.astype(np.complex64), sofs, offset


# the geometries of test_plframe_gpu.GEOMS, restated: n_slots 360 / 240 / 180 / 144 / 90 / 36 / 60, each with and without pilots
GEOM_PLSCS = [plsc_of(mc, sh, p) for mc, sh in [(4, 0), (13, 0), (18, 0), (24, 0), (4, 1), (0, 0), (13, 1)] for p in (0, 1)]
ES_N0 = (None, 10.0, 3.0, 0.0)
ACM_PLSCS = [plsc_of(4, 0, 1), plsc_of(13, 1, 0), plsc_of(0, 0, 0), plsc_of(13, 0, 0), plsc_of(4, 1, 1), plsc_of(4, 1, 1),
             plsc_of(18, 1, 1), plsc_of(0, 0, 0), plsc_of(4, 1, 0), plsc_of(4, 1, 1), plsc_of(24, 1, 0), plsc_of(4, 1, 1), plsc_of(4, 1, 1)]
RESTRICTED = [plsc_of(4, 1, 1), plsc_of(13, 1, 0), plsc_of(0, 0, 0), plsc_of(4, 0, 1), plsc_of(13, 0, 0), plsc_of(18, 1, 1),
              plsc_of(4, 1, 0), plsc_of(24, 1, 0)]
SHORT_QPSK = plsc_of(4, 1, 1)

# seed of every stream: the first of base, base + 1, ... for which the model alone passes the guard of test_plsync_model.py
# (no visited metric within its bound of a threshold, no soft decision within its bound of a tie), found by running that test
SEED_STEP = {'ccm-16-0-fixed': 1, 'ccm-16-0-decode': 38, 'ccm-17-3-decode': 2, 'ccm-17-0-fixed': 1, 'ccm-17-0-decode': 2,
             'ccm-52-0-fixed': 1, 'ccm-52-0-decode': 2, 'ccm-53-0-decode': 1, 'ccm-72-0-fixed': 2, 'ccm-72-0-decode': 5,
             'ccm-73-0-decode': 1, 'ccm-96-0-decode': 2, 'ccm-97-3-decode': 1, 'ccm-97-0-fixed': 12, 'ccm-97-0-decode': 3,
             'ccm-18-0-fixed': 1, 'ccm-54-0-fixed': 1, 'ccm-55-0-fixed': 1, 'ccm-55-0-decode': 1}


def cases():
    """Every (name, stream arguments, tracker arguments) the GPU tests run. Tracker arguments: fixed_plsc, unlock_thresh,
    coherent, soft, enabled."""
    out = []
    for i, p in enumerate(GEOM_PLSCS):
        nf = 4 if M.pls_parse(p)["plframe_len"] > 20000 else 6
        for es in ES_N0:
            name = f"ccm-{p}-{'clean' if es is None else int(es)}"
            stream = dict(plscs=[p] * nf, es_n0_db=es, gold=(0, 5, 131071)[i % 3])
            out.append((name + "-fixed", stream, dict(fixed_plsc=p)))
            out.append((name + "-decode", stream, dict()))
    acm = dict(plscs=ACM_PLSCS, es_n0_db=10.0)
    for coherent, soft in ((1, 1), (1, 0), (0, 0)):
        out.append((f"acm-{coherent}{soft}", acm, dict(coherent=coherent, soft=soft)))
    out.append(("acm-restricted", acm, dict(enabled=RESTRICTED)))
    out.append(("acm-3dB", dict(plscs=ACM_PLSCS, es_n0_db=3.0), dict()))
    for ut in (1, 2, 3):
        out.append((f"removed-{ut}", dict(plscs=[SHORT_QPSK] * 12, es_n0_db=10.0, removed=(5, 6)), dict(unlock_thresh=ut)))
        out.append((f"removed-{ut}-fixed", dict(plscs=[SHORT_QPSK] * 12, es_n0_db=10.0, removed=(5, 6)),
                    dict(unlock_thresh=ut, fixed_plsc=SHORT_QPSK)))
    return out


E2E = {"e2e-qpsk": dict(modcod=4, short=1, rate="C1_2", es_n0_db=6.0), "e2e-8psk": dict(modcod=14, short=0, rate="C3_4", es_n0_db=12.0)}
E2E_FRAMES, E2E_GOLD = 9, 5


def e2e_payload(name):
    """(sent BBFRAME bytes (nf, kbch / 8), XFECFRAME symbols (nf, n)) of an end-to-end stream: random bytes through the BCH and
    LDPC encoders of the test library, QPSK or 8PSK mapping. Needs the built library (code parameters) but no device."""
    import fec_testlib as T
    from dvbs2rx_amd import capi, get_fec_info
    e = E2E[name]
    framesize = capi.FECFRAME_SHORT if e["short"] else capi.FECFRAME_NORMAL
    fi = get_fec_info(capi.STANDARD_DVBS2, framesize, e["rate"])
    m, prim = T.BCH_FIELDS[framesize]
    ob = T.OracleBch(m, prim, fi["bch_t"], fi["bch_n"])
    rng = np.random.default_rng(61 + e["modcod"])
    sent = rng.integers(0, 256, (E2E_FRAMES, fi["bch_k"] // 8), dtype=np.uint8)
    cw = T.ldpc_encode(fi["table"], np.unpackbits(ob.encode_bytes(sent), axis=1))
    if e["modcod"] <= 11:
        syms = ((1 - 2.0 * cw[:, 0::2]) + 1j * (1 - 2.0 * cw[:, 1::2])) * np.sqrt(0.5)
    else:
        rows = cw.shape[1] // 3
        syms = T.map_8psk(np.stack([cw[:, a:a + rows] for a in (0, rows, 2 * rows)], axis=-1))
    return sent, syms


def extra_cases():
    """The streams of the GPU tests that are not compared record by record in test_search_records_equal_the_model but whose
    decisions those tests still assert: the metric test's stream (searched in short calls), the gather streams at an even and an
    odd offset, and the two end-to-end streams (stream key `payload`: XFECFRAMEs from e2e_payload; `scale`: amplitude)."""
    out = [("metric-stream", dict(plscs=[SHORT_QPSK] * 3 + [plsc_of(13, 1, 0)] * 2, es_n0_db=10.0, offset=1234, scale=0.8), dict())]
    for off in (700, 701):
        out.append((f"gather-{off}", dict(plscs=ACM_PLSCS, es_n0_db=10.0, offset=off, gold=E2E_GOLD), dict()))
    for name, e in E2E.items():
        out.append((name, dict(plscs=[plsc_of(e["modcod"], e["short"], 1)] * E2E_FRAMES, es_n0_db=e["es_n0_db"], offset=1777, gold=E2E_GOLD,
                               phase=2.1, foffset=2e-4, payload=name), dict()))
    return out


def all_cases():
    return cases() + extra_cases()


def base_seed(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000


def build_case(name, stream, trk, seed_step=None):
    """(x, sofs, model records, consumed, state, visits, decode log) of one case"""
    step = SEED_STEP.get(name, 0) if seed_step is None else seed_step
    stream = dict(stream)
    scale, payload = stream.pop("scale", None), stream.pop("payload", None)
    sent = None
    if payload is not None:
        sent, stream["data"] = e2e_payload(payload)
    x, sofs, _ = make_stream(seed=base_seed(name) + step, **stream)
    if scale is not None:
        x = (x * scale).astype(np.complex64)
    met, bound = metric(x)
    log = []
    dec = make_decoder(x, trk.get("coherent", 1), trk.get("soft", 1), trk.get("enabled"), log)
    recs, consumed, state, visits = track(met, dec, trk.get("unlock_thresh", 3), trk.get("fixed_plsc", -1), trk.get("max_frames"))
    return dict(x=x, sofs=sofs, sent=sent, met=met, bound=bound, recs=recs, consumed=consumed, state=state, visits=visits, log=log)


def guard(c):
    """number of visited metrics within their bound of the threshold they were compared with, and of unclear PLSC decisions"""
    met, bound, near = c["met"], c["bound"], 0
    for v in c["visits"]:
        if v[0] == "u":
            near += int((np.abs(met[v[1]:v[2]] - THRESHOLD_U) <= bound[v[1]:v[2]]).sum())
        else:
            near += int(abs(met[v[1]] - THRESHOLD_L) <= bound[v[1]])
    return near, sum(1 for _, clear in c["log"] if not clear)
