"""The float64 model of the PLFRAME front end (tests/plframe_model.py) against the known answers of the reference's own
unit tests (tests/golden/pl_kat.json), and the library's host-only entries against the model. No device needed."""
import ctypes as C

import numpy as np
import pytest

import plframe_model as M
from dvbs2rx_amd import capi, plheader_symbols, pls_parse

KAT = M.KAT


def signs(pairs):
    return np.array([(a + 1j * b) * M.S for a, b in pairs])


def with_last_sof(plsc_syms):
    """a 90-symbol header whose last 65 symbols are (last SOF symbol, 64 given symbols)."""
    return np.concatenate([M.map_bpsk(M.SOF_BITS), plsc_syms])


def test_sof_symbols_and_mapping_kats():
    q = KAT["qa_pi2_bpsk"]
    assert np.allclose(M.map_bpsk(M.SOF_BITS), signs(q["sof_symbol_signs"]), atol=1e-15)
    # derotate_bpsk: 0, 0, 1, 1 -> +1, +1, -1, -1
    s = signs(q["pi2bpsk_to_bpsk"]["symbol_signs"])
    assert np.allclose((s * M.ROT[np.arange(4) & 1]).real, q["pi2bpsk_to_bpsk"]["expected"], atol=1e-12)
    m = q["map_first_bit_one"]
    assert np.allclose(M.map_bpsk(M.word_bits(int(m["word"], 16), m["n"])), signs(m["symbol_signs"]))
    # demap_bpsk / demap_bpsk_diff of the all-ones word
    d = q["demapping_range"]
    syms = np.where(M.J64 & 1, signs([d["symbol_signs_odd"]])[0], signs([d["symbol_signs_even"]])[0])
    assert np.allclose(M.map_bpsk(M.SOF_BITS)[-1], signs([d["last_sof_symbol_signs"]])[0])
    for coherent in (True, False):
        bits = M.hard_bits(with_last_sof(syms), coherent)[0]
        for e in d["expected"]:
            assert np.array_equal(bits[:e["n"]], M.word_bits(int(e["word"], 16), e["n"]))


def test_plsc_encode_and_decode_kats():
    q = KAT["qa_pl_signaling"]
    e = q["plsc_encode"]
    assert M.CW[e["plsc"]] ^ M.SCR == int(e["codeword_xor_scrambler"], 16)
    d = q["plsc_decode"]
    x = with_last_sof(M.map_bpsk(M.word_bits(int(d["scrambled_word"], 16))))
    for coherent, soft in d["modes"]:
        info = M.pls_parse(int(M.plsc_decode(x, coherent, soft)[0]))
        assert {k: info[k] for k in d["expected"]} == d["expected"]


@pytest.mark.parametrize("coherent,soft", [(1, 1), (1, 0), (0, 0), (0, 1)])
def test_plsc_round_trip_all_modes(coherent, soft):
    rng = np.random.default_rng(5)
    x = np.stack([M.plheader(p) for p in range(128)])
    assert M.plsc_decode(x, coherent, soft).tolist() == list(range(128))
    # a common phase does not matter: the header is de-rotated by its SOF phase first
    xr = x * np.exp(1j * rng.uniform(-np.pi, np.pi, (128, 1)))
    assert M.plsc_decode(xr, coherent, soft).tolist() == list(range(128))


def test_plsc_parsing():
    q = KAT["qa_pl_signaling"]["parsing"]
    for modcod in range(q["modcod_min"], q["modcod_max"] + 1):
        for short in (0, 1):
            for pilots in (0, 1):
                plsc = (modcod << 2) | (short << 1) | pilots
                info = M.pls_parse(int(M.plsc_decode(M.plheader(plsc))[0]))
                assert (info["modcod"], info["short_fecframe"], info["has_pilots"]) == (modcod, short, pilots)
    for plsc in range(4):  # the dummy frame has no pilots whatever bit 0 says
        info = M.pls_parse(plsc)
        assert info["modcod"] == q["dummy_modcod"] and info["has_pilots"] == q["dummy_has_pilots"] and info["n_slots"] == 36
        assert info["plframe_len"] == 37 * 90
    assert M.pls_parse((4 << 2) | 1)["plframe_len"] == 361 * 90 + 22 * 36 and M.pls_parse((4 << 2) | 1)["n_pilots"] == 22
    assert M.pls_parse((13 << 2) | 3)["n_slots"] == 60 and M.pls_parse((13 << 2) | 3)["n_pilots"] == 3


@pytest.mark.parametrize("soft", [0, 1])
def test_reed_muller_corrects_15_errors(soft):
    rng = np.random.default_rng(11)
    t = KAT["qa_reed_muller"]["max_correctable_errors"]
    for p in range(128):
        bits = M.CW_BITS[p] ^ M.SCR_BITS
        bits[rng.choice(64, t, replace=False)] ^= 1
        x = with_last_sof(M.map_bpsk(bits))
        assert M.plsc_decode(x, 1, soft)[0] == p


@pytest.mark.parametrize("soft", [0, 1])
def test_reed_muller_subset(soft):
    sub = KAT["qa_reed_muller"]["subset"]["enabled"]
    for p in range(128):
        got = int(M.plsc_decode(M.plheader(p), 1, soft, enabled=sub)[0])
        # (what the reference's test asks; the soft decoder may answer with a disabled index, see the quirk below)
        assert (got == p) if p in sub else (got != p and (soft or got in sub))
    # list ORDER decides ties of the hard decoder: codeword 1 is at distance 32 from both 64 and 96
    assert M.plsc_decode(M.plheader(1), 1, 0, enabled=[96, 64])[0] == 96
    assert M.plsc_decode(M.plheader(1), 1, 0, enabled=[64, 96])[0] == 64
    # soft quirk: every enabled metric negative -> a disabled entry (0.0) wins, the first one
    x = M.plheader(2) * 1.0
    x[M.SOF_LEN:] *= -1  # the complement of codeword 2 = codeword 2 ^ all-ones row: metric of 2 is -64
    assert M.plsc_decode(x, 1, 1, enabled=[2])[0] == 0


def test_library_plheader_symbols_and_parse():
    for p in range(128):
        got = plheader_symbols(p)
        assert got.dtype == np.complex64
        assert np.array_equal(got, M.plheader(p).astype(np.complex64)), p
        want = M.pls_parse(p)
        assert pls_parse(p) == {k: want[k] for k in ("plframe_len", "payload_len", "xfecframe_len", "n_slots", "n_pilots", "n_mod")}, p
    buf = np.zeros(180, np.float32)
    assert capi.lib.dvbs2_plheader_symbols(128, buf.ctypes.data) == capi.EINVAL
    assert capi.lib.dvbs2_plheader_symbols(-1, buf.ctypes.data) == capi.EINVAL
    assert capi.lib.dvbs2_plheader_symbols(0, None) == capi.EINVAL
    assert capi.lib.dvbs2_pls_parse(128, None, None, None, None, None, None) == capi.EINVAL


def test_create_checks_its_arguments_before_the_device():
    """A bad PLSC, a reserved MODCOD or a bad gold code is refused with a message on any machine."""
    h = C.c_void_p()
    for gold, plsc in ((0, 128), (0, -1), (0, 29 << 2), (0, (31 << 2) | 3), (1 << 18, 4), (-1, 4)):
        assert capi.lib.dvbs2_plframe_create(C.byref(h), gold, plsc, 4, 0) == capi.EINVAL, (gold, plsc)
        assert capi.lib.dvbs2_last_error() and not h.value
    assert capi.lib.dvbs2_plframe_params(None, None, None, None, None, None, None) == capi.EINVAL


def test_signal_generator_round_trip():
    """make_plframes against the model's own estimators: noise-free frames give back the phase and the offset."""
    rng = np.random.default_rng(3)
    plsc, gold = (13 << 2) | 3, 5  # 8PSK-sized short frame with pilots: 60 slots, 3 pilot blocks
    x, _ = M.make_plframes(plsc, gold, 3, rng, None, phase=0.7, foffset=1e-4)
    est, tol, aux = M.estimates(x, plsc, gold, [1, 1, 0])
    assert np.allclose(est["fine_foffset"][:2], 1e-4, atol=1e-9) and est["fine_foffset"][2] == 0
    assert est["fine_valid"].tolist() == [1, 1, 0]
    assert abs(M.angdiff(est["sof_phase"][0], 0.7 + M.PI2 * 1e-4 * 12.5)) < 1e-3
    assert M.plsc_decode(x).tolist() == [plsc] * 3
    out, _ = M.payload_step(x, plsc, gold, [1, 1, 0], est, tol)
    # de-rotated back onto the QPSK points, up to the 45 symbols between the middle of the header and its end (0.028 rad)
    assert np.abs(np.abs(out[:2].real) - M.S).max() < 0.03
