"""float32 restatement of the PL framer (dvbs2_plframer_*): swaps and np.negative only, the header from plframe_model.plheader rounded
once to float32, Rn from plframe_model.scrambling_rn, the layout from plframe_model.pls_parse. Everything is (re, im) float32 pairs,
so that a result can be compared as uint32."""
import numpy as np

import plframe_model as M

S32 = np.float32(0.70710678118654752440)
RESERVED = (29, 30, 31)


def layout(plscs):
    """dict of in_offset, out_offset (one per frame), in_syms, out_syms: the running sums of xfecframe_len (0 for a dummy frame) and
    plframe_len."""
    ino, outo, i, o = [], [], 0, 0
    for p in plscs:
        info = M.pls_parse(int(p))
        ino.append(i)
        outo.append(o)
        i += 0 if info["dummy_frame"] else info["xfecframe_len"]
        o += info["plframe_len"]
    return dict(in_offset=np.array(ino, np.int64), out_offset=np.array(outo, np.int64), in_syms=i, out_syms=o)


def header(plsc):
    """(90, 2) float32"""
    h = M.plheader(int(plsc))
    return np.stack([h.real, h.imag], -1).astype(np.float32)


def scramble(pairs, rn):
    """(n, 2) float32 times j^rn: rn 0 (a, b), 1 (-b, a), 2 (-a, -b), 3 (b, -a)."""
    a, b = pairs[:, 0], pairs[:, 1]
    na, nb = np.negative(a), np.negative(b)
    re = np.choose(rn, [a, nb, na, b])
    im = np.choose(rn, [b, a, nb, na])
    return np.stack([re, im], -1)


def descramble(pairs, rn):
    """The rule of pl_payload_kernel: rn 0 (x, y), 1 (y, -x), 2 (-x, -y), 3 (-y, x)."""
    x, y = pairs[:, 0], pairs[:, 1]
    nx, ny = np.negative(x), np.negative(y)
    return np.stack([np.choose(rn, [x, y, nx, ny]), np.choose(rn, [y, nx, ny, x])], -1)


def pilot_mask(info):
    """True at the payload indices of pilot symbols."""
    k = np.arange(info["payload_len"])
    return (info["n_pilots"] > 0) & (k % M.PERIOD >= M.PERIOD - M.PBLK) & (k // M.PERIOD < info["n_pilots"])


def frame(plsc, gold, data):
    """One PLFRAME (plframe_len, 2) float32. data: (xfecframe_len, 2) float32; ignored (may be None) for a dummy frame."""
    info = M.pls_parse(int(plsc))
    pay = np.empty((info["payload_len"], 2), np.float32)
    pay[:] = S32
    if not info["dummy_frame"]:
        pay[~pilot_mask(info)] = np.asarray(data, np.float32).reshape(info["xfecframe_len"], 2)
    rn = M.scrambling_rn(gold, info["payload_len"])
    return np.concatenate([header(plsc), scramble(pay, rn)])


def frames(plscs, gold, data, closing_plsc=-1):
    """The PLFRAMEs of a sequence back to back (+ the closing header): (n, 2) float32. data: (in_syms, 2) float32, the XFECFRAMEs
    of the non-dummy frames back to back."""
    lay = layout(plscs)
    data = np.asarray(data, np.float32).reshape(-1, 2)
    assert data.shape[0] == lay["in_syms"]
    parts = []
    for p, i in zip(plscs, lay["in_offset"]):
        info = M.pls_parse(int(p))
        parts.append(frame(p, gold, None if info["dummy_frame"] else data[i:i + info["xfecframe_len"]]))
    if closing_plsc >= 0:
        parts.append(header(closing_plsc))
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def planted_data(rng, n):
    """(n, 2) random normal float32 with 0.0, -0.0 and a denormal planted in both components."""
    d = rng.normal(size=(n, 2)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-41, -1e-41], np.float32)
    for j, v in enumerate(special):
        d[(3 + 7 * j) % n, 0] = v
        d[(5 + 11 * j) % n, 1] = v
        d[n - 1 - j, j & 1] = v
    return d
