"""The rotator rows in Python integers (include/dvbs2_fec_hip.h, "rotator rows"; notes/rotator_rows.md): a stream's record, the phase
rule, the rebase, the control rule with its one conversion, the conversion of an increment as csrc/rotator_turns.h does it in extended
precision, and one rotated sample in float64 with the rotator's derived bound. The record's phase is an exact integer here as on the
device, so the bound is the single rotator's (tests/plcoarse_model.py, Rotator.work) WITHOUT its term for the rounding of an increment:
that rounding happens once, when a record is made, and is part of the record. No bound here was tuned to what the device returns."""
from fractions import Fraction

import numpy as np

import plcoarse_model as R
import plframe_model as M

MASK = (1 << 64) - 1
TWO_PI_LITERAL = Fraction(6283185307179586476925286766559005768, 10 ** 36)  # the decimal literal of csrc/rotator_turns.h


# ------------------------------------------------------------------ the conversion of an increment (csrc/rotator_turns.h)
def _rn64(x):
    """the Fraction x rounded to a 64-bit significand, ties to even: one operation of the extended type"""
    if x == 0:
        return x
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1  # 2^e <= x < 2^(e + 1)
    scale = Fraction(2) ** (63 - e)
    y = x * scale
    n = y.numerator // y.denominator
    r = y - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return sign * Fraction(n) / scale


def inc_turns(inc):
    """rotator_inc_turns(inc), operation by operation: the quotient by 2 pi (the literal rounded to the type), minus its floor, scaled
    by 2^64 (exact), rounded half away from zero, 2^64 taken as 0"""
    t = _rn64(Fraction(float(inc)) / _rn64(TWO_PI_LITERAL))
    t = _rn64(t - (t.numerator // t.denominator))  # floorl; the difference rounds when t is negative and tiny
    s = t * (1 << 64)
    n = s.numerator // s.denominator
    if s - n >= Fraction(1, 2):
        n += 1
    return 0 if n >= 1 << 64 else n


# ------------------------------------------------------------------ the record and its phase
def state(phase=0, inc=0, index=0, reserved=0):
    return dict(phase=phase & MASK, inc=inc & MASK, index=index, reserved=reserved)


def from_records(recs):
    """numpy records of ROTATOR_STATE -> list of dicts of Python ints"""
    return [state(int(r["phase"]), int(r["inc"]), int(r["index"]), int(r["reserved"])) for r in recs]


def to_records(states, dtype):
    out = np.zeros(len(states), dtype)
    for r, st in zip(out, states):
        r["phase"], r["inc"], r["index"], r["reserved"] = st["phase"], st["inc"], st["index"], st["reserved"]
    return out


def phase_at(st, m):
    """the phase of absolute sample m, any m"""
    return (st["phase"] + (m - st["index"]) * st["inc"]) & MASK


def rebase(st, at):
    st["phase"], st["index"] = phase_at(st, at), at


def retune(st, at, inc):
    rebase(st, at)
    st["inc"] = inc_turns(inc)


# ------------------------------------------------------------------ the control rule
def adjust_turns(estimate, scale):
    """(delta, applies): d = float64(float32(estimate)) * scale, applies = finite and |d| < 0.5, delta = rint(d * 2^64) as an integer"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float64(np.float32(estimate)) * np.float64(scale)
    if not np.isfinite(d) or not abs(d) < 0.5:
        return 0, False
    return int(np.rint(d * 2.0 ** 64)), True


def control(offsets, max_slots, coarse_foffset, coarse_corrected, new_est, fine_foffset, fine_valid, coarse_scale, fine_scale, at, states):
    """the rule over one pass; changes `states` in place; returns (applied, delta), one entry per stream"""
    applied, deltas = [], []
    for s, st in enumerate(states):
        kind, e = 0, 0.0
        for i in range(max(offsets[s], 0), min(offsets[s + 1], max_slots)):
            if new_est[i] != 0 and coarse_corrected[i] == 0:
                kind, e = 1, coarse_foffset[i]
            elif coarse_corrected[i] != 0 and fine_valid is not None and fine_valid[i] != 0:
                kind, e = 2, fine_foffset[i]
        delta = 0
        if kind:
            delta, applies = adjust_turns(e, coarse_scale if kind == 1 else fine_scale)
            if applies:
                rebase(st, at)
                st["inc"] = (st["inc"] - delta) & MASK
            else:
                kind = -1
        applied.append(kind)
        deltas.append(delta)
    return applied, deltas


# ------------------------------------------------------------------ one call in float64
def rotate(x, st, base_index):
    """(exact output complex128, per-sample bound on |device - exact|) of the samples x of one row whose first has the absolute index
    base_index. The device's phase error: 2^-26 turns (the upper 32 bits as a float in half-turns) + 2^-32 turns (the lower 32 bits
    dropped); sincospif and the complex product as in plcoarse_model.Rotator.work."""
    x = np.asarray(x, np.complex128)
    ph = [phase_at(st, base_index + i) for i in range(x.size)]
    frac = np.array([p >> 4 for p in ph], np.float64) / 2.0 ** 60
    out = x * np.exp(1j * M.PI2 * frac)
    dphi = M.PI2 * (2.0 ** -26 + 2.0 ** -32)
    return out, 1.01 * np.abs(x) * (dphi + np.sqrt(2.0) * R.SINCOS_ERR + 4.2 * R.U)
