"""CPU: the float32 model of the PL framer (tests/plframer_model.py) against the float64 signal generator the receive-side tests have
used so far, and against the descrambling rule of pl_payload_kernel. Needs neither the library nor a device."""
import numpy as np
import pytest

import plframe_model as M
import plframer_model as F
import plsync_model as PS


def _data(plsc, nf, seed):
    info = M.pls_parse(plsc)
    rng = np.random.default_rng(seed)
    if info["dummy_frame"]:
        return info, None
    return info, F.planted_data(rng, nf * info["xfecframe_len"])


@pytest.mark.parametrize("plsc", PS.GEOM_PLSCS)
@pytest.mark.parametrize("gold", [0, 5])
def test_model_equals_make_plframes(plsc, gold):
    """make_plframes goes through complex128 and (1j) ** rn, hence a bound and not bits: 2^-23, the float32 spacing below 2, per
    component. ((1j) ** rn is off the axis by about 1e-16, far below half a float32 step of any deviate, so the bound holds for the
    few deviates above 2 as well.)"""
    nf = 2
    info, d = _data(plsc, nf, 100 + plsc)
    if info["dummy_frame"]:
        d64 = np.full((nf, info["xfecframe_len"]), complex(F.S32, F.S32))  # a dummy frame's payload is (S, S)
        got = F.frames([plsc] * nf, gold, np.zeros((0, 2), np.float32), closing_plsc=plsc)
    else:
        d64 = (d[:, 0].astype(np.float64) + 1j * d[:, 1].astype(np.float64)).reshape(nf, info["xfecframe_len"])
        got = F.frames([plsc] * nf, gold, d, closing_plsc=plsc)
    want, trail = M.make_plframes(plsc, gold, nf, np.random.default_rng(1), data=d64, trailing=True)
    want = np.concatenate([want.reshape(-1), trail])
    assert got.shape == (nf * info["plframe_len"] + 90, 2)
    w = np.stack([want.real, want.imag], -1).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - w) <= 2.0 ** -23).all()


@pytest.mark.parametrize("plsc", PS.GEOM_PLSCS)
def test_descrambling_and_dropping_the_pilots_returns_the_data_exactly(plsc):
    gold = 7
    info, d = _data(plsc, 1, 200 + plsc)
    fr = F.frame(plsc, gold, d)
    assert fr.shape == (info["plframe_len"], 2)
    assert np.array_equal(F.bits(fr[:90]), F.bits(F.header(plsc)))
    rn = M.scrambling_rn(gold, info["payload_len"])
    pay = F.descramble(fr[90:], rn)
    mask = F.pilot_mask(info)
    assert mask.sum() == 36 * info["n_pilots"]
    if info["dummy_frame"]:
        assert (pay == F.S32).all()
        return
    # pilots come back as (S, S); -(-x) restores every bit, so the data come back as bits, the planted zeros and denormals included
    assert (pay[mask] == F.S32).all()
    assert np.array_equal(F.bits(pay[~mask]), F.bits(d))


def test_layout_is_the_running_sums():
    lay = F.layout(PS.ACM_PLSCS)
    infos = [M.pls_parse(p) for p in PS.ACM_PLSCS]
    assert lay["out_offset"].tolist() == np.concatenate([[0], np.cumsum([i["plframe_len"] for i in infos])[:-1]]).tolist()
    assert lay["in_syms"] == sum(i["xfecframe_len"] for i in infos if not i["dummy_frame"])
    assert all(o % 2 == 0 for o in lay["in_offset"].tolist() + lay["out_offset"].tolist())
