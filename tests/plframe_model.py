"""float64 model of the PLFRAME front end, written from the reference (lib/pl_signaling.cc, lib/reed_muller.cc,
lib/pi2_bpsk.cc, lib/pl_freq_sync.cc, lib/plsync_cc_impl.cc) with the constants of tests/golden/pl_kat.json.
Deliberately the slow way round: a 128-codeword table for the PLSC (no transform), direct sums for the phases."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "pl_kat.json")))
SOF = int(KAT["sof_word"], 16)
SOF_LEN = KAT["sof_len"]
SCR = int(KAT["plsc_scrambler"], 16)
G = [int(x, 16) for x in KAT["rm_generator_rows"]]
PERIOD, PBLK, SLOT, HLEN = KAT["pilot_block_period"], KAT["pilot_block_len"], KAT["slot_len"], KAT["plheader_len"]
S = np.sqrt(2.0) / 2.0
PI2 = 2.0 * np.pi


def pls_parse(plsc):
    """pls_info_t::parse (lib/pl_signaling.cc:19-61)."""
    modcod, short, pilots = plsc >> 2, (plsc >> 1) & 1, plsc & 1
    dummy = modcod == 0
    if dummy:
        pilots = 0
    n_mod, n_slots = KAT["modcod_other"]["n_mod"], KAT["modcod_other"]["n_slots"]
    for r in KAT["modcod_rule"]:
        if r["modcod_min"] <= modcod <= r["modcod_max"]:
            n_mod, n_slots = r["n_mod"], r["n_slots"]
    if short and not dummy:
        n_slots //= KAT["short_divides_slots_by"]
    n_pilots = ((n_slots - 1) >> 4) if pilots else 0
    plframe_len = (n_slots + 1) * SLOT + PBLK * n_pilots
    return dict(plsc=plsc, modcod=modcod, short_fecframe=short, has_pilots=pilots, dummy_frame=int(dummy), n_mod=n_mod,
                n_slots=n_slots, n_pilots=n_pilots, plframe_len=plframe_len, payload_len=plframe_len - HLEN,
                xfecframe_len=n_slots * SLOT)


def rm_codeword(plsc):
    """lib/reed_muller.cc:72-96: index 2 i + b7, bits (y1 y1' y2 y2' ...), y' = y xor b7, first bit in bit 63."""
    i, code32 = plsc >> 1, 0
    for row in range(6):
        if i & (0x20 >> row):
            code32 ^= G[row]
    b = (~code32 & 0xFFFFFFFF) if plsc & 1 else code32
    w = 0
    for t in range(32):
        w |= ((code32 >> t) & 1) << (2 * t + 1)
        w |= ((b >> t) & 1) << (2 * t)
    return w


def word_bits(w, n=64, width=64):
    return np.array([(w >> (width - 1 - j)) & 1 for j in range(n)], np.uint8)


CW = [rm_codeword(p) for p in range(128)]
CW_BITS = np.stack([word_bits(c) for c in CW])             # unscrambled, for hard decoding
SCR_BITS = word_bits(SCR)
IMG = 1.0 - 2.0 * (CW_BITS ^ SCR_BITS[None, :])            # Euclidean images of the SCRAMBLED codewords (lib/pl_signaling.cc:95-98)
SOF_BITS = word_bits(SOF, SOF_LEN, SOF_LEN)
ROT = np.array([S - 1j * S, -S - 1j * S])                   # lib/pi2_bpsk.cc:57-60
J64 = np.arange(64)


def map_bpsk(bits):
    """lib/pi2_bpsk.cc:18-43 (index 0 is even)."""
    bits = np.asarray(bits)
    k = np.arange(bits.shape[-1])
    base = np.where(k & 1, -S + 1j * S, S + 1j * S)
    return base * (1.0 - 2.0 * bits)


def plheader_bits(plsc):
    return np.concatenate([SOF_BITS, CW_BITS[plsc] ^ SCR_BITS])


def plheader(plsc):
    return map_bpsk(plheader_bits(plsc))


_XY = []


def scrambling_rn(gold, n):
    """ETSI EN 302 307-1 clause 5.5.4: x(i+18) = x(i+7) + x(i), y(i+18) = y(i+10) + y(i+7) + y(i+5) + y(i);
    z_n(i) = x((i + n) mod (2^18 - 1)) + y(i); Rn(i) = 2 z_n((i + 131072) mod (2^18 - 1)) + z_n(i)."""
    P = (1 << 18) - 1
    if not _XY:
        x, y = [0] * P, [0] * P
        x[0] = 1
        y[:18] = [1] * 18
        for i in range(P - 18):
            x[i + 18] = x[i + 7] ^ x[i]
            y[i + 18] = y[i + 10] ^ y[i + 7] ^ y[i + 5] ^ y[i]
        _XY.extend([np.array(x, np.uint8), np.array(y, np.uint8)])
    x, y = _XY
    i = np.arange(n)
    z = lambda k: x[(k % P + gold) % P] ^ y[k % P]  # noqa: E731
    return (2 * z(i + 131072) + z(i)).astype(np.uint8)


def wrap(d):
    """into [-pi, pi] the way the reference does it: one correction (lib/pl_freq_sync.cc:280-285)."""
    d = np.asarray(d, np.float64).copy()
    d[d > np.pi] -= PI2
    d[d < -np.pi] += PI2
    return d


def angdiff(a, b):
    """a - b modulo 2 pi, in (-pi, pi]."""
    return (np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % PI2 - np.pi


def sum_and_bound(terms):
    """angle of a sum of L terms, and the bound of a float32 sum in any order plus atan2f against it:
    4 L 2^-24 sum|term| / |sum term| + 1e-6 rad. Also returns |sum| / L."""
    L = terms.shape[-1]
    s = terms.sum(-1)
    tol = 4.0 * L * 2.0 ** -24 * np.abs(terms).sum(-1) / np.abs(s) + 1e-6
    return np.angle(s), tol, np.abs(s) / L


# ------------------------------------------------------------------ PLSC decoding (lib/pl_signaling.cc:114-167)
def derotated_header(x):
    """closed-loop derotate_plheader (lib/pl_freq_sync.cc:429-436)."""
    x = np.asarray(x, np.complex128)[..., :HLEN]
    sof_phase = np.angle((x[..., :SOF_LEN] * np.conj(map_bpsk(SOF_BITS))).sum(-1))
    return x * np.exp(-1j * sof_phase)[..., None]


def enabled_order(enabled):
    return list(range(128)) if enabled is None or len(enabled) == 0 else [int(e) for e in enabled]


def soft_metrics(x, enabled=None):
    """(n, 128) float64 dot products; entries of disabled codewords stay 0.0 (lib/reed_muller.cc:203-209)."""
    y = derotated_header(x)
    sd = (y[..., SOF_LEN:] * ROT[J64 & 1]).real
    m = sd @ IMG.T
    mask = np.zeros(128, bool)
    mask[enabled_order(enabled)] = True
    m[..., ~mask] = 0.0
    return m


def soft_tau(x):
    """2^-16 sum_k |x_k| over the 64 PLSC symbols."""
    return 2.0 ** -16 * np.abs(np.asarray(x, np.complex128)[..., SOF_LEN:HLEN]).sum(-1)


def hard_bits(x, coherent):
    """Scrambled hard decisions and the decision variables with their eligibility scale |x|^2."""
    y = derotated_header(x)
    if coherent:
        dv = (y[..., SOF_LEN:] * ROT[J64 & 1]).real                       # lib/pi2_bpsk.cc:45-74
        bits = (dv < 0).astype(np.uint8)
        scale = np.abs(y[..., SOF_LEN:]) ** 2
    else:
        dv = (np.conj(y[..., SOF_LEN:]) * y[..., SOF_LEN - 1:HLEN - 1]).imag  # lib/pi2_bpsk.cc:165-176
        t = (dv < 0).astype(np.uint8) ^ (J64 & 1).astype(np.uint8)
        bits = (np.cumsum(t, axis=-1) & 1).astype(np.uint8)
        scale = np.maximum(np.abs(y[..., SOF_LEN:]), np.abs(y[..., SOF_LEN - 1:HLEN - 1])) ** 2
    return bits, dv, scale


def hard_decode_bits(rx_scrambled, enabled=None):
    """minimum Hamming distance, FIRST minimum in list order, strict < (lib/reed_muller.cc:128-141)."""
    rx = np.atleast_2d(rx_scrambled) ^ SCR_BITS[None, :]
    order = np.array(enabled_order(enabled))
    dist = (rx[:, None, :] != CW_BITS[None, order, :]).sum(-1)  # every distance, in list order
    return order[np.argmin(dist, axis=1)].astype(np.uint8)      # argmin: the first minimum


def plsc_decode(x, coherent=True, soft=True, enabled=None):
    x = np.atleast_2d(x)
    if coherent and soft:
        return np.argmax(soft_metrics(x, enabled), axis=-1).astype(np.uint8)  # first maximum
    return hard_decode_bits(hard_bits(x, coherent)[0], enabled)


def hard_eligible(x, coherent):
    """False where a decision variable is below 2^-20 |x|^2: float32 rounding may flip that decision."""
    _, dv, scale = hard_bits(np.atleast_2d(x), coherent)
    return (np.abs(dv) >= 2.0 ** -20 * scale).all(-1)


# ------------------------------------------------------------------ phases and fine frequency offset
def estimates(frames, plsc, gold, coarse_corrected, coarse_foffset=None, trailing=None):
    """frames (nf, plframe_len) complex. Returns values and per-value bounds as dicts of arrays."""
    info = pls_parse(plsc)
    x = np.asarray(frames, np.complex128)
    nf, npil, flen = x.shape[0], info["n_pilots"], info["plframe_len"]
    h = plheader(plsc)
    sof, sof_tol, sof_q = sum_and_bound(x[:, :SOF_LEN] * np.conj(h[:SOF_LEN]))
    hph, hph_tol, hph_q = sum_and_bound(x[:, :HLEN] * np.conj(h))
    est = dict(sof_phase=sof, plheader_phase=hph)
    tol = dict(sof_phase=sof_tol, plheader_phase=hph_tol)
    quality = [sof_q, hph_q]
    cc = np.asarray(coarse_corrected) != 0
    fine = np.zeros(nf)
    fine_tol = np.zeros(nf)
    valid = np.zeros(nf, np.int32)
    margin = np.full(nf, np.inf)  # distance of the wrapped differences from +-pi
    if npil:
        rn = scrambling_rn(gold, info["payload_len"])
        a0, a0_tol, a0_q = sum_and_bound(x[:, HLEN - PBLK:HLEN] * np.conj(h[HLEN - PBLK:]))
        ang, atol = [a0], [a0_tol]
        quality.append(a0_q)
        for i in range(npil):
            k = (i + 1) * PERIOD - PBLK
            p = x[:, HLEN + k:HLEN + k + PBLK] * (-1j) ** rn[k:k + PBLK]   # lib/pl_descrambler.cc:56-58
            a, t, q = sum_and_bound(p)
            ang.append(wrap(a - np.pi / 4.0))
            atol.append(t)
            quality.append(q)
        ang, atol = np.stack(ang, 1), np.stack(atol, 1)
        est["pilot_phase"], tol["pilot_phase"] = ang[:, 1:], atol[:, 1:]
        raw = ang[:, 1:] - ang[:, :-1]
        d = wrap(raw.reshape(-1)).reshape(raw.shape)
        margin = np.abs(np.pi - np.abs(raw)).min(1)
        fine = np.where(cc, d.sum(1) / (PI2 * PERIOD * npil), 0.0)
        fine_tol = (atol[:, 1:] + atol[:, :-1]).sum(1) / (PI2 * PERIOD * npil)
        valid = cc.astype(np.int32)
    else:
        est["pilot_phase"], tol["pilot_phase"] = np.zeros((nf, 0)), np.zeros((nf, 0))
        nxt, nxt_tol = np.zeros(nf), np.zeros(nf)
        have = np.zeros(nf, bool)
        nxt[:-1], nxt_tol[:-1], have[:-1] = hph[1:], hph_tol[1:], True
        if trailing is not None:
            a, t, q = sum_and_bound(np.asarray(trailing, np.complex128)[None, :HLEN] * np.conj(h))
            nxt[-1], nxt_tol[-1], have[-1] = a[0], t[0], True
            quality.append(q)
        cf = np.asarray(coarse_foffset, np.float32).astype(np.float64)
        ok = cc & have & (np.abs(cf) <= 1.0 / (2.0 * flen))                # lib/pl_freq_sync.cc:325-327
        raw = nxt - hph
        margin = np.where(ok, np.abs(np.pi - np.abs(raw)), np.inf)
        fine = np.where(ok, wrap(raw) / (PI2 * flen), 0.0)
        fine_tol = (nxt_tol + hph_tol) / (PI2 * flen)
        valid = ok.astype(np.int32)
    est["fine_foffset"], tol["fine_foffset"], est["fine_valid"] = fine, fine_tol, valid
    return est, tol, dict(min_quality=min(float(q.min()) for q in quality), wrap_margin=margin, info=info)


def payload_step(frames, plsc, gold, coarse_corrected, est, tol):
    """handle_payload (lib/plsync_cc_impl.cc:644-653, :725-795) in float64 with the given phases; returns the XFECFRAMEs and
    the per-symbol bound |x| (tol_phase + 2 pi tol_foffset 1440 + 2^-21)."""
    info = pls_parse(plsc)
    x = np.asarray(frames, np.complex128)
    nf, npil, ns = x.shape[0], info["n_pilots"], info["n_slots"]
    rn = scrambling_rn(gold, info["payload_len"])
    o = np.arange(ns * SLOT)
    blk = (o // SLOT) // 16 if npil else np.zeros_like(o)
    k = o + blk * PBLK
    d = x[:, HLEN + k] * (-1j) ** rn[k][None, :]
    cc = (np.asarray(coarse_corrected) != 0)[:, None]
    inc = np.where(cc, PI2 * est["fine_foffset"][:, None], 0.0)
    use_pilot = cc & (blk > 0)[None, :]
    if npil:
        pil = est["pilot_phase"][:, np.maximum(blk - 1, 0)]
        ptol = tol["pilot_phase"][:, np.maximum(blk - 1, 0)]
    else:
        pil = ptol = np.zeros((nf, o.size))
    theta0 = np.where(use_pilot, pil, est["plheader_phase"][:, None])
    ttol = np.where(use_pilot, ptol, tol["plheader_phase"][:, None])
    steps = np.where(use_pilot, o[None, :] - blk[None, :] * 16 * SLOT, o[None, :])
    out = d * np.exp(-1j * (theta0 + inc * steps))
    bound = np.abs(d) * (ttol + PI2 * tol["fine_foffset"][:, None] * 1440.0 + 2.0 ** -21)
    return out, bound


# ------------------------------------------------------------------ signal generator
def make_plframes(plsc, gold, nf, rng, es_n0_db=None, phase=0.0, foffset=0.0, data=None, trailing=False):
    """nf PLFRAMEs of the PLSC back to back (+ the next PLHEADER when trailing): PLHEADER, data slots with the unmodulated
    pilots (1 + j) / sqrt(2) every 16 slots, PL scrambling of the payload, then one phasor exp(j (phase + 2 pi foffset n))
    running over the whole stream, then AWGN. data: (nf, xfecframe_len) complex, default random QPSK."""
    info = pls_parse(plsc)
    ns, npil, flen = info["n_slots"], info["n_pilots"], info["plframe_len"]
    if data is None:
        data = ((1 - 2.0 * rng.integers(0, 2, (nf, ns * SLOT))) + 1j * (1 - 2.0 * rng.integers(0, 2, (nf, ns * SLOT)))) * S
    rn = scrambling_rn(gold, info["payload_len"])
    o = np.arange(ns * SLOT)
    blk = (o // SLOT) // 16 if npil else np.zeros_like(o)
    payload = np.full((nf, info["payload_len"]), S + 1j * S, np.complex128)
    payload[:, o + blk * PBLK] = data
    payload *= (1j) ** rn[None, :]
    h = plheader(plsc)
    tx = np.concatenate([np.broadcast_to(h, (nf, HLEN)), payload], axis=1).reshape(-1)
    if trailing:
        tx = np.concatenate([tx, h])
    n = np.arange(tx.size)
    ph = np.asarray(phase, np.float64)
    if ph.ndim:  # one phase per frame on top of the running offset
        ph = np.concatenate([np.repeat(ph, flen), np.full(tx.size - nf * flen, ph[-1])])
    rx = tx * np.exp(1j * (ph + PI2 * foffset * n))
    if es_n0_db is not None:
        n0 = 10.0 ** (-es_n0_db / 10.0)
        rx = rx + np.sqrt(n0 / 2.0) * (rng.normal(size=rx.size) + 1j * rng.normal(size=rx.size))
    rx = rx.astype(np.complex64)
    return (rx[:nf * flen].reshape(nf, flen), rx[nf * flen:]) if trailing else (rx.reshape(nf, flen), None)
