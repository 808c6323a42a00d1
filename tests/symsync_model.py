"""Models of the symbol timing recovery loop (reference lib/symbol_sync_cc_impl.cc:283-401), for tests/test_symsync_model.py
(no device) and tests/test_symsync_gpu.py:
  (a) exact=True   the loop with float64 interpolants, error and gains;
  (b) exact=False  a restatement in the device's arithmetic: float32 interpolants -- the polyphase dot product summed as the kernel
      sums it (lane j of 32 takes taps j, j + 32, ... in ascending order, then a xor butterfly 16, 8, 4, 2, 1), the Farrow
      interpolants in the reference's expression order --, the float32 error, the float32 products K1 e and K2 e widened to double,
      and the double arithmetic of the counter. The device is compared with (b) bit for bit.
Both keep the history, the state and the stop rules of include/dvbs2_fec_hip.h, so a stream may be cut into calls."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "symsync_kat.json")))
U = 2.0 ** -24
F32, F64 = np.float32, np.float64
GUARD = 0.01           # a strobe whose n_subfilt * mu (model (a)) is this close to an integer may take the other subfilter in (b)
GUARD_SHARE = 0.05     # at most this share of a run (expected: 2 GUARD)
MAX_JUMP = 1 << 30
# |mu of (b) - mu of (a)|, the largest value measured on each closed-loop set below (test_symsync_model.py prints it); the tolerance
# of a set is four times its own measurement
MU_SEEN = {"poly-sps2": 1.18e-7, "poly-sps4": 1.21e-7, "lin-sps2": 4.57e-8, "lin-sps4": 1.08e-7, "quad-sps2": 8.09e-8,
           "quad-sps4": 5.70e-8, "cub-sps2": 4.83e-8, "cub-sps4": 7.29e-8, "poly-sps2-fast": 1.13e-5}


def mu_tol(name):
    return 4 * MU_SEEN[name]


def loop_constants(sps, loop_bw, damping, rolloff):
    """(Kp, K1, K2) as float32, every line of :166-198 rounded to float once with C++'s promotions"""
    loop_bw, damping, rolloff = F32(loop_bw), F32(damping), F32(rolloff)
    L = F32(1e3)
    with np.errstate(divide="ignore", invalid="ignore"):
        C = F32(np.sin(np.pi * F64(rolloff) / 2) / (4 * np.pi * F64(F32(1) - (rolloff * rolloff / F32(4)))))
        dx = F32(2.0 / F64(L))
        dy = F32(F64(F32(8) * C) * np.sin(2 * np.pi / F64(L)))
        Kp = F32(dy / dx)
        bn_t = F32(loop_bw / F32(sps))
        theta = F32(F64(bn_t) / (F64(damping) + (1.0 / F64(F32(4) * damping))))
        den = F32(F32(F32(1) + F32(F32(F32(2) * damping) * theta)) + F32(theta * theta))
        k1 = F32(F32(F32(F32(4) * damping) * theta) / den)
        k2 = F32(F32(F32(4) * F32(theta * theta)) / den)
        return Kp, F32(k1 / F32(Kp * F32(-1))), F32(k2 / F32(Kp * F32(-1)))


def geometry(sps, rrc_delay, n_subfilt, interp):
    L = 2 * sps * rrc_delay + 1
    return L, (L - 1) // 2, (L - 1 if interp == 0 else 1 if interp == 1 else 3) + sps // 2


def rrc(t, a):
    """root raised cosine impulse response at t symbols, float64; t = 0 and |t| = 1 / (4 a) by their limits"""
    t = np.asarray(t, F64)
    out = np.empty_like(t)
    z = t == 0.0
    s = (np.abs(np.abs(4.0 * a * t) - 1.0) < 1e-9) & (a > 0)
    r = ~(z | s)
    out[z] = 1.0 - a + 4.0 * a / np.pi
    if a > 0:
        out[s] = a / np.sqrt(2.0) * ((1.0 + 2.0 / np.pi) * np.sin(np.pi / (4.0 * a)) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / (4.0 * a)))
    tr = t[r]
    out[r] = (np.sin(np.pi * tr * (1.0 - a)) + 4.0 * a * tr * np.cos(np.pi * tr * (1.0 + a))) / (np.pi * tr * (1.0 - 16.0 * a * a * tr * tr))
    return out


def rc(t, a):
    """raised cosine impulse response at t symbols"""
    t = np.asarray(t, F64)
    s = np.abs(np.abs(2.0 * a * t) - 1.0) < 1e-9
    den = np.where(s, 1.0, 1.0 - (2.0 * a * t) ** 2)
    return np.where(s, np.pi / 4.0 * np.sinc(1.0 / (2.0 * a)) if a > 0 else 0.0, np.sinc(t) * np.cos(np.pi * a * t) / den)


def prototype(sps, rolloff, rrc_delay, n_subfilt):
    """the RRC prototype at n_subfilt * sps samples per symbol, float64, summing to n_subfilt"""
    a = float(F32(rolloff))
    poly = n_subfilt * sps
    n = 2 * poly * rrc_delay + 1
    h = rrc((np.arange(n) - (n - 1) // 2) / poly, a)
    return h * n_subfilt / h.sum()


def taps(sps, rolloff, rrc_delay, n_subfilt):
    """the bank [n_subfilt, subfilt_len] as float32: zero pad, subfilter i = taps i + j n_subfilt, each flipped (:82-110)"""
    L = geometry(sps, rrc_delay, n_subfilt, 0)[0]
    h = np.zeros(n_subfilt * L)
    p = prototype(sps, rolloff, rrc_delay, n_subfilt)
    h[:p.size] = p
    return np.ascontiguousarray(h.reshape(L, n_subfilt).T[:, ::-1]).astype(F32)


C3 = [F32(1.0 / 6), F32(-.5), F32(.5), F32(-(1.0 / 6))]
C2 = [F32(0.0), F32(.5), F32(-1.0), F32(.5)]
C1 = [F32(-(1.0 / 6)), F32(1.0), F32(-.5), F32(-(1.0 / 3))]
Q2 = [F32(.5), F32(-.5), F32(-.5), F32(.5)]
Q1 = [F32(-.5), F32(1.5), F32(-.5), F32(-.5)]
LANE = np.arange(32)


class SymSync:
    def __init__(self, sps=2, loop_bw=0.01, damping=1.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp_method=0, exact=False, bank=None):
        self.sps, self.interp, self.ns, self.exact = sps, interp_method, n_subfilt, exact
        self.L, self.D, self.H = geometry(sps, rrc_delay, n_subfilt, interp_method)
        self.Kp, self.K1, self.K2 = loop_constants(sps, loop_bw, damping, rolloff)
        self.bank = taps(sps, rolloff, rrc_delay, n_subfilt) if bank is None else np.asarray(bank, F32)
        self.bank64 = self.bank.astype(F64)
        # taps per lane: row q holds taps 32 q .. 32 q + 31, zero beyond the subfilter
        P = -(-self.L // 32)
        self.lanes = np.zeros((n_subfilt, P, 32), F32)
        self.lanes.reshape(n_subfilt, -1)[:, :self.L] = self.bank
        self.P = P
        self.step = 1.0 / float(F32(sps))
        self.reset()

    def reset(self):
        self.vi, self.cnt, self.mu, self.jump, self.init, self.status, self.n_read = 0.0, 1.0 - self.step, 0.0, self.sps, False, 0, 0
        self.last = np.complex64(0) if not self.exact else 0j
        self.hist = np.zeros(self.H, np.complex64)
        self.terms = []  # per strobe of the last work(): sum |term| of the output interpolant, float64

    def state(self):
        return dict(vi=self.vi, cnt=self.cnt, mu=self.mu, n_read=self.n_read, last_xi=self.last, jump=self.jump, init=int(self.init),
                    status=self.status)

    # ---- interpolants: (value, sum of |term| per component)
    def _poly(self, v, b):
        p = np.floor(float(self.ns) * self.mu)
        idx = int(p) if 0 <= p < self.ns else (self.ns - 1 if p >= self.ns else 0)
        seg = v[b + 2 - self.L:b + 2]
        if self.exact:
            t = seg.astype(np.complex128) * self.bank64[idx]
            return t.sum(), max(np.abs(t.real).sum(), np.abs(t.imag).sum())
        x = np.zeros(self.P * 32, np.complex64)
        x[:self.L] = seg
        x = x.reshape(self.P, 32)
        c = self.lanes[idx]
        ar, ai = np.zeros(32, F32), np.zeros(32, F32)
        for q in range(self.P):  # float32 products and sums, one rounding each
            ar = ar + x[q].real * c[q]
            ai = ai + x[q].imag * c[q]
        for m in (16, 8, 4, 2, 1):
            ar = ar + ar[LANE ^ m]
            ai = ai + ai[LANE ^ m]
        return np.complex64(complex(ar[0], ai[0])), 0.0

    def _farrow(self, v, b):
        if self.exact:
            x = [complex(v[b + 1 - i]) for i in range(4)]
            mu = self.mu
            tot = sum(max(abs(z.real), abs(z.imag)) for z in x)
            if self.interp == 1:
                return mu * x[0] + (1 - mu) * x[1], tot
            if self.interp == 2:
                v2 = sum(x[i] * float(Q2[i]) for i in range(4))
                v1 = sum(x[i] * float(Q1[i]) for i in range(4))
                return (mu * v2 + v1) * mu + x[2], tot
            c3, c1 = [1 / 6, -.5, .5, -1 / 6], [-1 / 6, 1.0, -.5, -1 / 3]
            v3 = sum(x[i] * c3[i] for i in range(4))
            v2 = sum(x[i] * float(C2[i]) for i in range(4))
            v1 = sum(x[i] * c1[i] for i in range(4))
            return ((mu * v3 + v2) * mu + v1) * mu + x[2], tot
        m = F32(self.mu)
        out = []
        for comp in ("real", "imag"):
            x = [F32(getattr(v[b + 1 - i], comp)) for i in range(4)]
            if self.interp == 1:
                out.append(F32(F32(m * x[0]) + F32(F32(F32(1) - m) * x[1])))
                continue
            v3, v2, v1 = F32(0), F32(0), F32(0)
            for i in range(4):
                if self.interp == 2:
                    v2 = F32(v2 + F32(x[i] * Q2[i]))
                    v1 = F32(v1 + F32(x[i] * Q1[i]))
                else:
                    v3 = F32(v3 + F32(x[i] * C3[i]))
                    v2 = F32(v2 + F32(x[i] * C2[i]))
                    v1 = F32(v1 + F32(x[i] * C1[i]))
            if self.interp == 2:
                out.append(F32(F32(F32(F32(m * v2) + v1) * m) + x[2]))
            else:
                out.append(F32(F32(F32(F32(F32(F32(m * v3) + v2) * m) + v1) * m) + x[2]))
        return np.complex64(complex(out[0], out[1])), 0.0

    def work(self, samples, max_out=None):
        """one call: returns (symbols, absolute strobe indices, mu per symbol, consumed, status)"""
        x = np.asarray(samples, np.complex64)
        max_out = x.size if max_out is None else max_out
        self.terms = []
        if self.status or (not self.init and x.size < 2):
            return np.zeros(0, np.complex128 if self.exact else np.complex64), np.zeros(0, np.int64), np.zeros(0), 0, self.status
        H, mid = self.H, self.sps // 2
        v = np.concatenate([self.hist, x])
        total = v.size
        interp = self._poly if self.interp == 0 else self._farrow
        n = H - 1
        if not self.init:
            self.last = complex(v[H]) if self.exact else v[H]
            self.init = True
            n += 2
        out, idx, mus = [], [], []
        with np.errstate(all="ignore"):
            while n + self.jump < total and len(out) < max_out:
                n += self.jump
                m_k = n - 1
                o, t = interp(v, m_k)
                zc, _ = interp(v, m_k - mid)
                out.append(o)
                idx.append(self.n_read + m_k - H)
                mus.append(self.mu)
                self.terms.append(t)
                if self.exact:
                    e = zc.real * (self.last.real - o.real) + zc.imag * (self.last.imag - o.imag)
                    vp, dvi = float(self.K1) * e, float(self.K2) * e
                else:
                    e = F32(F32(zc.real * F32(self.last.real - o.real)) + F32(zc.imag * F32(self.last.imag - o.imag)))
                    vp, dvi = float(F32(self.K1 * e)), float(F32(self.K2 * e))
                self.last = o
                self.vi = self.vi + dvi
                pi_out = vp + self.vi
                W1, W2 = self.step + pi_out, self.step + self.vi
                if W1 != W1 or W2 != W2:
                    self.status = 2
                    break
                if not (W1 > 0.0 and W2 > 0.0):
                    self.status = 1
                    break
                jd = np.floor(F64(self.cnt - W1) / F64(W2)) + 2.0
                if not (1.0 <= jd <= MAX_JUMP):
                    self.status = 3
                    break
                self.jump = int(jd)
                if self.jump > 1:
                    cb = self.cnt - W1 - ((self.jump - 2) * W2)
                    self.mu = float(F64(cb) / F64(W2))
                    self.cnt = cb - W2 + 1
                else:
                    self.mu = float(F64(self.cnt) / F64(W1))
                    self.cnt = self.cnt - W1 + 1
        consumed = n + 1 - H
        if consumed > 0:
            self.hist = v[consumed:consumed + H].copy()
        self.n_read += consumed
        return (np.array(out, np.complex128 if self.exact else np.complex64), np.array(idx, np.int64), np.array(mus, F64), consumed,
                self.status)


def map_tag_offsets(tag_offsets, n_read, strobe_idx, n_written, strobe_offset):
    """general_work's tag placement (:471-487) for strobe indices RELATIVE to the call's input buffer: each tag goes to the
    first strobe at or past offset - n_read + strobe_offset; returns (placed output offsets, tags left pending)"""
    placed, pending = [], []
    for t in tag_offsets:
        i = int(np.searchsorted(strobe_idx, t - n_read + strobe_offset, side="left"))
        if i < len(strobe_idx):
            placed.append(n_written + i)
        else:
            pending.append(t)
    return placed, pending


# ------------------------------------------------------------------ inputs
def kat_vectors():
    return [(v, np.array([complex(a, b) for a, b in v["in"]], np.complex64), np.array([complex(a, b) for a, b in v["out"]])) for v in KAT["vectors"]]


def kat_cfg(v):
    return {k: v[k] for k in ("sps", "loop_bw", "damping", "rolloff", "rrc_delay", "n_subfilt", "interp_method")}


def open_loop_input():
    o = KAT["open_loop"]
    syms = np.array(o["symbols"], np.complex64)
    x = np.zeros(syms.size * o["sps"], np.complex64)
    x[::o["sps"]] = syms
    return x, syms


def qpsk_stream(seed, sps, nsyms, rolloff, ppm, noise, matched, tau0=0.3, delay=8):
    """QPSK symbols through an RRC pulse (matched=False: the polyphase bank is the matched filter) or an RC pulse (matched=True:
    what a matched filter in front of a Farrow interpolator leaves), sampled at sps (1 + ppm 1e-6) samples per symbol with a
    start offset of tau0 symbols, plus noise per component. Returns (samples complex64, symbols)."""
    rng = np.random.default_rng(seed)
    a = ((1 - 2.0 * rng.integers(0, 2, nsyms)) + 1j * (1 - 2.0 * rng.integers(0, 2, nsyms))) * np.sqrt(0.5)
    n = int((nsyms - 1) * sps)
    t = np.arange(n) / (sps * (1.0 + ppm * 1e-6)) + tau0
    k0 = np.floor(t).astype(int)
    x = np.zeros(n, np.complex128)
    pulse = rc if matched else rrc
    for d in range(-delay, delay + 1):
        k = k0 + d
        ok = (k >= 0) & (k < nsyms)
        x[ok] += a[k[ok]] * pulse(t[ok] - k[ok], rolloff)
    if not matched:  # unit symbols after a filter of unit DC gain matched to the pulse
        x /= np.sum(rrc(np.arange(-delay * sps, delay * sps + 1) / sps, rolloff) ** 2) / np.sum(rrc(np.arange(-delay * sps, delay * sps + 1) / sps, rolloff))
    x += noise * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return x.astype(np.complex64), a


# (name, configuration, stream arguments): every closed-loop random input the GPU tests use. A clock offset of 500 ppm over 1100
# symbols moves the sampling instant by more than one sample, so every run wraps mu and takes jumps other than sps.
# Why 1100 symbols and no more: the difference in mu between (a) and (b) is a random walk fed by the float32 roundings (measured on a
# 12000-symbol polyphase run: 3.5e-9 after 10 strobes, 2.9e-8 after 100, 5.6e-7 after 1000, 2.9e-6 after 2900). The first strobe at
# which the two select different subfilters -- expected once 2 n_subfilt times the sum of these differences reaches 1, near 3000
# strobes for 128 subfilters, and seen at strobe 2930 of that run -- changes the error by a whole subfilter step; the two loops then
# follow different trajectories 1e-3 apart in mu and never close again, and a comparison of outputs says nothing after it. At 1100
# strobes the expected number of such strobes is below 0.1. The device is compared with (b) bit for bit, which has no such limit.
CLOSED_SETS = [(f"{('poly', 'lin', 'quad', 'cub')[m]}-sps{sps}",
                dict(sps=sps, loop_bw=0.01, damping=1.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp_method=m),
                dict(seed=100 + 10 * m + sps, sps=sps, nsyms=1100, rolloff=0.2, ppm=500.0, noise=0.1, matched=m != 0))
               for m in range(4) for sps in (2, 4)]
CLOSED_SETS.append(("poly-sps2-fast", dict(sps=2, loop_bw=0.05, damping=0.707, rolloff=0.35, rrc_delay=5, n_subfilt=32, interp_method=0),
                    dict(seed=8, sps=2, nsyms=1100, rolloff=0.35, ppm=-500.0, noise=0.05, matched=False)))
# a loop bandwidth far too wide: the integrator runs away and W2 turns non-positive (the stop case of the GPU tests)
STOP_CFG = dict(sps=2, loop_bw=0.12, damping=1.0, rolloff=0.2, rrc_delay=5, n_subfilt=128, interp_method=1)
STOP_STREAM = dict(seed=5, sps=2, nsyms=600, rolloff=0.2, ppm=0.0, noise=0.3, matched=True)


def closed_set(name):
    for n, cfg, st in CLOSED_SETS:
        if n == name:
            return cfg, qpsk_stream(**st)[0]
    raise KeyError(name)


def output_bound(model_a):
    """Per strobe of model (a)'s last work(): the bound 4 L 2^-24 sum |term| on |(b) - (a)| per component. Polyphase: L = subfilt_len
    and the terms are the tap products. Farrow: L = 4 taps and sum |term| is the sum over the four samples of max(|re|, |im|)."""
    t = np.asarray(model_a.terms, F64)
    return 4 * (model_a.L if model_a.interp == 0 else 4) * U * t
