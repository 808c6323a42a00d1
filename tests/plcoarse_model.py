"""float64 model of the coarse frequency offset estimate (reference lib/pl_freq_sync.cc:93-199 with the mode rule of
lib/plsync_cc_impl.cc:567-606) and of the rotator (lib/rotator_cc_impl.cc:36-128), with the bound of a float32 evaluation of
each and the points at which such an evaluation may legitimately decide otherwise. Deliberately the slow way round: direct
sums per lag, Python integers for the rotator's phase. No bound here was tuned to what the device returns; each is derived
where it is computed from u = 2^-24 (float32 unit roundoff) and the documented accuracy of the math library."""
from fractions import Fraction

import numpy as np

import plframe_model as M

U = 2.0 ** -24
RANGE = 3.3875e-4              # fine_foffset_corr_range, lib/pl_freq_sync.h:18
ATAN2F_ERR = 2.0 ** -21        # atan2f: 2 ulp at |angle| <= pi (ulp(pi) = 2^-22), twice the 1 ulp HIP documents for it
SINCOS_ERR = 2.0 ** -22        # sincospif: 2 ulp at |value| <= 1 (ulp <= 2^-23 below 1), twice the documented 1 ulp
MAX_LPL = 33282                # MAX_PLFRAME_LEN, the spacing of lib/qa_pl_freq_sync.cc:107


def weights(full):
    """lib/pl_freq_sync.cc:74-85, in double"""
    L = 89 if full else 25
    m = np.arange(L, dtype=np.float64)
    return 3.0 * ((2 * L + 1.0) ** 2 - (2 * m + 1.0) ** 2) / (((2 * L + 1.0) ** 2 - 1) * (2 * L + 1))


def autocorr(x90, plsc, full):
    """(R[0..L] complex128 with R[0] = 0, A[0..L]): R[m] = sum_k z[k+m] conj(z[k]) with z = x conj(h) sqrt(2) (the scale the
    device uses: +-1 +- j taps), A[m] = sum_k |z[k+m]| |z[k]|, the magnitude sum the rounding bound needs."""
    N = 90 if full else 26
    z = np.asarray(x90[:N], np.complex128) * np.conj(M.plheader(plsc)[:N]) * np.sqrt(2.0)
    R, A = np.zeros(N, np.complex128), np.zeros(N)
    for m in range(1, N):
        R[m] = np.sum(z[m:] * np.conj(z[:N - m]))
        A[m] = np.sum(np.abs(z[m:]) * np.abs(z[:N - m]))
    return R, A


class Coarse:
    """freq_sync::estimate_coarse with its state, plus the mode rule of its caller. step(x90, plsc) returns
    dict(foffset, corrected, new_est, full) and, when new_est, `bound` and `eligible`."""

    def __init__(self, period, known_plsc=False):
        self.period, self.known = period, known_plsc
        self.reset()

    def reset(self):
        self.i_frame, self.f, self.corrected = 0, 0.0, False
        self.R, self.A = np.zeros(90, np.complex128), np.zeros(90)

    def step(self, x90, plsc):
        full = self.corrected or self.known
        N = 90 if full else 26
        R, A = autocorr(x90, plsc, full)
        self.R[:N] += R
        self.A[:N] += A
        self.i_frame += 1
        out = dict(full=full, new_est=False)
        if self.i_frame >= self.period:
            self.i_frame = 0
            out.update(self._finish(full), new_est=True)
            self.R[:], self.A[:] = 0, 0
        out.update(foffset=self.f, corrected=self.corrected)
        return out

    def _finish(self, full):
        L = 89 if full else 25
        N = L + 1
        R, A, w = self.R[:N], self.A[:N], weights(full)
        # --- float32 error of R[m]. z: one float add per component, relative u. A component of R[m] is a sum of at most
        # 2 N products over the frame (two per term), carried on over `period` frames: at most 2 N + period additions on top
        # of the product and the z roundings (3 u), in whatever order. Standard bound: (n_add + 3) u sum |products|
        # <= (2 N + period + 3) u A[m] per component, times sqrt(2) for the complex magnitude.
        dR = np.sqrt(2.0) * (2 * N + self.period + 3) * U * A
        absR = np.abs(R)
        ok = absR[1:] > 2.0 * dR[1:]  # otherwise the float32 angle is not confined
        # --- angles: a perturbation dR of R turns its angle by at most asin(dR / |R|) <= (pi / 2) dR / |R|; atan2f adds its own
        dth = np.zeros(N)
        with np.errstate(divide="ignore", invalid="ignore"):
            dth[1:] = np.where(ok, (np.pi / 2) * dR[1:] / absR[1:], np.pi) + ATAN2F_ERR
        th = np.zeros(N)
        th[1:] = np.arctan2(R[1:].imag, R[1:].real)
        # --- differences: float subtraction of two angles (|result| <= 2 pi: u 2 pi), the wrap in double rounded to float
        # (|result| <= pi: u pi)
        d = th[1:] - th[:-1]
        dd = dth[1:] + dth[:-1] + 3 * np.pi * U
        d = np.where(d > np.pi, d - 2 * np.pi, np.where(d < -np.pi, d + 2 * np.pi, d))
        # an unwrapped difference within dd of +-pi may wrap the other way in float32 (equivalently: the wrapped one near +-pi)
        wrap_safe = bool(np.all(np.pi - np.abs(d) > dd))
        # --- weighted sum: the weights are float32-rounded (u), each product rounds (u), the sum of L terms in any order
        # (L u): (L + 2) u sum |w d|; the division by 2 pi in double and the rounding to float: u |f|
        s = float(np.sum(w * d))
        df = (float(np.sum(w * dd)) + (L + 2) * U * float(np.sum(np.abs(w * d)))) / (2 * np.pi) + U * abs(s / (2 * np.pi))
        f = min(max(s / (2 * np.pi), -0.5), 0.5)
        eligible = bool(ok.all()) and wrap_safe and 0.5 - abs(f) > df and abs(abs(f) - RANGE) > df
        self.f, self.corrected = f, abs(f) < RANGE
        return dict(bound=df, eligible=eligible)


def run(headers, plscs, period, known_plsc=False, state=None):
    """a sequence of headers ([n, >= 90] complex) through one Coarse; returns per-frame arrays and the per-window lists"""
    c = state or Coarse(period, known_plsc)
    fo, cc, ne, full, bound, elig = [], [], [], [], [], []
    for x, p in zip(headers, plscs):
        o = c.step(x, int(p))
        fo.append(o["foffset"]); cc.append(int(o["corrected"])); ne.append(int(o["new_est"])); full.append(int(o["full"]))
        bound.append(o.get("bound", 0.0)); elig.append(o.get("eligible", True))
    return dict(foffset=np.array(fo), corrected=np.array(cc, np.int32), new_est=np.array(ne, np.int32), full=np.array(full, np.int32),
                bound=np.array(bound), eligible=np.array(elig, bool))


def comparable(m):
    """(indices of the frames to compare, number of windows, number of ineligible windows): everything up to the first
    ineligible window; after it the mode may differ, so the rest of the sequence is not compared."""
    win = np.flatnonzero(m["new_est"])
    bad = [i for i in win if not m["eligible"][i]]
    stop = bad[0] if bad else len(m["new_est"])
    # the frames of the ineligible window before its last one still carry the previous, comparable state
    return np.arange(stop), len(win), len(bad)


# ------------------------------------------------------------------ inputs
def rotated_header(plsc, foffset, phase0, amp=1.0):
    """lib/qa_pl_freq_sync.cc:25-34 on the noiseless PLHEADER, as float32 symbols"""
    n = np.arange(90)
    return (amp * M.plheader(plsc) * np.exp(1j * (phase0 + M.PI2 * foffset * n))).astype(np.complex64)


QA_PLSC = (21 << 2) | (1 << 1)                        # lib/qa_pl_freq_sync.cc:49-52, :74
QA_OFFSETS = (-0.23, -0.13, 0.03, 0.19, 0.25)         # :63
QA_CORRECTED = (-3.26e-4, -1e-4, -1e-5, 1e-5, 1e-4, 3.26e-4)  # :144


def qa_unit_period(f):
    return np.stack([rotated_header(QA_PLSC, f, np.pi)])


def qa_period_two(f):
    """:100-133: two headers MAX_PLFRAME_LEN apart at f, then two at -f with the phase carried on"""
    ph, out = np.pi, []
    out.append(rotated_header(QA_PLSC, f, ph))
    ph += MAX_LPL * M.PI2 * f
    out.append(rotated_header(QA_PLSC, f, ph))
    ph += MAX_LPL * M.PI2 * -f
    out.append(rotated_header(QA_PLSC, -f, ph))
    ph += MAX_LPL * M.PI2 * -f
    out.append(rotated_header(QA_PLSC, -f, ph))
    return np.stack(out)


# (name, seed, n_frames, Es/N0 in dB or None, cap on the share of ineligible windows). Seeds are plain; test_plcoarse_model
# checks with the model alone that each set stays inside its cap
RANDOM_SETS = [("clean", 11, 160, None, 0.0), ("20dB", 12, 160, 20.0, 0.0), ("10dB", 13, 160, 10.0, 0.0),
               ("3dB", 14, 320, 3.0, 0.01), ("0dB", 15, 320, 0.0, 0.01)]
PERIODS = (1, 2, 5, 32)


def random_set(seed, n, es_n0_db, period):
    """n headers in windows of `period`: within a window one offset (uniform in +-0.3) and one amplitude, every frame its own
    phase and PLSC (all 128 occur); AWGN of the given Es/N0 relative to the frame's amplitude."""
    rng = np.random.default_rng(seed * 100 + period)
    plscs = (np.arange(n) * 37 + int(rng.integers(0, 128))) % 128  # 37 is odd: a permutation of 0..127 per 128 frames
    xs = []
    for i in range(n):
        if i % period == 0:
            f, amp = rng.uniform(-0.3, 0.3), rng.uniform(0.3, 3.0)
        x = rotated_header(int(plscs[i]), f, rng.uniform(-np.pi, np.pi), amp).astype(np.complex128)
        if es_n0_db is not None:
            s = amp * np.sqrt(10.0 ** (-es_n0_db / 10.0) / 2.0)
            x = x + s * (rng.normal(size=90) + 1j * rng.normal(size=90))
        xs.append(x.astype(np.complex64))
    return np.stack(xs), plscs.astype(np.uint8)


def mode_switch_set():
    """offset 0.1 for 4 frames, 1e-4 for 6, 0.1 again for 5 (period 1, Es/N0 = 34 dB so that the SOF and the full estimate of
    one header differ by more than the float32 bound): SOF, then full from the frame AFTER the first small estimate, then SOF
    again from the frame after the first large one"""
    fs = [0.1] * 4 + [1e-4] * 6 + [0.1] * 5
    rng = np.random.default_rng(2)
    plscs = np.array([(7 * i + 3) % 128 for i in range(len(fs))], np.uint8)
    s = np.sqrt(10.0 ** -3.4 / 2.0)
    xs = [rotated_header(int(p), f, 0.3 + i).astype(np.complex128) + s * (rng.normal(size=90) + 1j * rng.normal(size=90))
          for i, (p, f) in enumerate(zip(plscs, fs))]
    return np.stack(xs).astype(np.complex64), plscs


def streaming_set():
    return random_set(77, 45, 10.0, 4)  # period 4 divides neither 1, 7 nor the rest (37)


# ------------------------------------------------------------------ rotator
def _pi_fixed(bits):
    """pi * 2^bits as an integer: Machin's formula in integer arithmetic"""
    one = 1 << (bits + 32)

    def atan_inv(q):
        t = one // q
        s, k, sign = t, 1, 1
        while t:
            t //= q * q
            k += 2
            sign = -sign
            s += sign * (t // k)
        return s
    return (16 * atan_inv(5) - 4 * atan_inv(239)) >> 32


FRAC = 160
TWO_PI = Fraction(2 * _pi_fixed(200), 1 << 200)
ONE = 1 << FRAC


def turns(inc):
    """inc radians as turns in 2^-FRAC units (the double `inc` taken exactly), modulo one turn"""
    return int(Fraction(float(inc)) / TWO_PI * ONE) % ONE


class Rotator:
    """rotator_cc::work with the phase as an exact integer. Equal offsets: scheduling order, the last one wins."""

    def __init__(self, inc=0.0):
        self.inc0 = inc
        self.reset()

    def reset(self):
        self.counter, self.phase, self.inc, self.absinc, self.queue, self.dropped = 0, 0, turns(self.inc0), abs(self.inc0), [], 0

    def set_phase_inc(self, inc):
        self.inc, self.absinc = turns(inc), abs(inc)

    def schedule(self, offset, inc):
        i = len(self.queue)
        while i > 0 and self.queue[i - 1][0] > offset:
            i -= 1
        self.queue.insert(i, (offset, inc))

    def segments(self, n):
        """advance over n samples; returns [(start, length, phase at start, inc, |inc| in radians)] relative to the call"""
        segs, done = [], 0
        while self.queue:
            off, inc = self.queue[0]
            if off < self.counter + done:
                self.queue.pop(0); self.dropped += 1
                continue
            if off >= self.counter + n:
                break
            self.queue.pop(0)
            items = off - self.counter - done
            if items:
                segs.append((done, items, self.phase, self.inc, self.absinc))
            self.phase = (self.phase + items * self.inc) % ONE
            done += items
            self.set_phase_inc(inc)
        if n - done:
            segs.append((done, n - done, self.phase, self.inc, self.absinc))
        self.phase = (self.phase + (n - done) * self.inc) % ONE
        self.counter += n
        return segs

    def seek(self, n):
        self.segments(n)

    def work(self, x):
        """(exact output complex128, per-sample bound on |device - exact|) for the device's phase representation:
        phase error <= 2^-26 turns (the upper 32 bits as a float: a value in [0.5, 1) half-turns has half-ulp 2^-25 half-turns)
                     + 2^-32 turns (the lower 32 bits dropped)
                     + k ((|inc| / 2 pi) 2^-63 + 2^-65) turns, k = samples since the segment's start: the increment is
                       converted once with a 64-bit significand (quotient and constant: relative 2^-63) and rounded to 2^-64
                       turns; the segment's start phase carries the same error of the earlier segments, bounded here by
                       charging k from the start of the CALL'S history: k = absolute sample index (an upper bound);
        |e^{j phi'} - e^{j phi}| <= |phi' - phi|; sin and cos each within SINCOS_ERR: sqrt(2) SINCOS_ERR on the phasor;
        the complex multiply: per component two products and one add, (1 + u)^2 - 1 < 2.1 u relative to |x| |phasor| ... each
        component's error <= 2.1 u (|a c| + |b s|) <= 2.1 u |x| sqrt(2); both components: 2.1 u |x| 2. The phasor's own modulus
        is within 1 + sqrt(2) SINCOS_ERR, absorbed by the factor 1.01."""
        x = np.asarray(x, np.complex128)
        n0 = self.counter
        out, bound = np.empty(x.size, np.complex128), np.empty(x.size)
        for start, length, ph, inc, absinc in self.segments(x.size):
            k = np.arange(length, dtype=object)
            p = (ph + k * inc) % ONE
            frac = np.array([int(v) >> (FRAC - 60) for v in p], np.float64) / 2.0 ** 60
            sl = slice(start, start + length)
            out[sl] = x[sl] * np.exp(1j * M.PI2 * frac)
            kabs = (n0 + start + np.arange(length)).astype(np.float64)
            dphi = M.PI2 * (2.0 ** -26 + 2.0 ** -32 + kabs * (max(absinc, 2 * np.pi) / M.PI2 * 2.0 ** -63 + 2.0 ** -65))
            bound[sl] = 1.01 * np.abs(x[sl]) * (dphi + np.sqrt(2.0) * SINCOS_ERR + 4.2 * U)
        return out, bound


# ------------------------------------------------------------------ the end-to-end point
E2E_FOFFSET, E2E_ES_N0_DB, E2E_SEED, E2E_OFFSET, E2E_PERIOD = 0.03, 15.0, 4242, 1501, 3


def e2e_stream():
    """(stream, SOF indices, sent BBFRAME bytes, PLSC): the short QPSK 1/2 pilot-mode frames of plsync_model's end-to-end
    case with a carrier offset of 0.03 cycles per symbol at Es/N0 = 15 dB"""
    import plsync_model as P
    e = P.E2E["e2e-qpsk"]
    plsc = P.plsc_of(e["modcod"], e["short"], 1)
    sent, syms = P.e2e_payload("e2e-qpsk")
    x, sofs, _ = P.make_stream([plsc] * P.E2E_FRAMES, E2E_SEED, es_n0_db=E2E_ES_N0_DB, offset=E2E_OFFSET, gold=P.E2E_GOLD, phase=0.7,
                               foffset=E2E_FOFFSET, data=syms)
    return x, sofs, sent, plsc


def e2e_model(x, sofs, plsc):
    """pass 1 (windows of E2E_PERIOD frames, known PLSC) over the headers, the last estimate f, the stream rotated by -f,
    pass 2 (period 1) over its headers"""
    p1 = run([x[s:s + 90] for s in sofs], [plsc] * len(sofs), E2E_PERIOD, True)
    f = p1["foffset"][-1]
    y = (x.astype(np.complex128) * np.exp(-1j * M.PI2 * f * np.arange(x.size))).astype(np.complex64)
    p2 = run([y[s:s + 90] for s in sofs], [plsc] * len(sofs), 1, True)
    return p1, f, p2
