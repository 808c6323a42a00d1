"""CPU: the models of the polyphase channelizer (tests/pfbch_model.py) against each other and against the library's host-only entries:
the float32 restatement within the derived bound of the double sum, cuts of a stream bit for bit, every channel against the
down-converter's float64 model, the count rule, the selection, the twiddle table and special values."""
import importlib.util
import math
import os

import numpy as np
import pytest

import ddc_model as DM
import pfbch_model as PM
import spectrum_model as SM
from dvbs2rx_amd import pfbch_geometry, pfbch_produce, pfbch_tile, pfbch_twiddles, spectrum_twiddles

F32 = np.float32


def signal(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex64)


def random_taps(seed, ntaps):
    return (np.random.default_rng(seed).normal(size=ntaps) / math.sqrt(ntaps)).astype(F32)


# ------------------------------------------------------------------ the float32 restatement under the bound
@pytest.mark.parametrize("M,D,ntaps", [(2, 2, 5), (4, 4, 33), (8, 4, 65), (8, 3, 40), (16, 16, 129), (64, 32, 513), (8, 8, 3)])
def test_float32_model_within_the_bound(M, D, ntaps):
    """|Y32 - Y64| <= sqrt(2) gamma_q S (1 + B) + B ||w||_2 per output (notes/pfbch.md). Normal inputs, normal taps / sqrt(ntaps). Measured
    here: 0.03-0.18 of the bound (the largest at M 2 with 5 taps). The bound is the one the stage was specified with; pfbch_model.bound
    says how it stands to Higham's theorem."""
    taps, x = random_taps(M + ntaps, ntaps), signal(D + ntaps, 200 * D + ntaps)
    y32, _ = PM.channelize32(taps, M, D, x)
    y64, S, w_norm = PM.channelize64(taps, M, D, x)
    b = PM.bound(M, ntaps, S, w_norm)
    err = np.abs(y32.astype(np.complex128) - y64)
    ratio = float((err / b[None, :]).max())
    print(f"M {M} D {D} ntaps {ntaps}: worst error / bound {ratio:.4f}, worst error {err.max():.3e}")
    assert y32.shape == (M, PM.produce(0, D, x.size)) and ratio <= 1.0


# ------------------------------------------------------------------ cuts
@pytest.mark.parametrize("M,D,ntaps", [(8, 3, 40), (16, 8, 5), (8, 4, 1), (8, 4, 21), (4, 1, 9), (256, 128, 4096)])
def test_cuts_give_the_bits_of_one_call(M, D, ntaps):
    """One call equals any cutting, bit for bit: cuts of 3 M + 1 (the position then is off the multiples of D and of M), 0, 1, D - 1, 5
    and the rest. D not dividing M, ntaps below M, one tap, ntaps no multiple of M, and the largest bank."""
    taps = random_taps(ntaps, ntaps)
    n = 3 * M + 1 + 5 + D + 12 * D + 3
    x = signal(M * D + ntaps, n)
    whole, hist_whole = PM.channelize32(taps, M, D, x)
    cuts = [3 * M + 1, 0, 1, D - 1, 5]
    assert (3 * M + 1) % M and (D == 1 or (3 * M + 1) % D)
    cuts.append(n - sum(cuts))
    parts, pos, hist = [], 0, None
    for c in cuts:
        y, hist = PM.channelize32(taps, M, D, x[pos:pos + c], pos, hist)
        assert y.shape == (M, PM.produce(pos, D, c))
        parts.append(y)
        pos += c
    assert pos == n and np.array_equal(PM.bits(np.concatenate(parts, axis=1)), PM.bits(whole))
    assert np.array_equal(PM.bits(hist), PM.bits(hist_whole))


# ------------------------------------------------------------------ against the down-converter
def test_every_channel_against_the_ddc_model():
    """Channel c is the down-converter from reset with phase_inc = -2 pi c / M, the same taps and D: within the sum of the two stages'
    bounds (the channelizer's above; the down-converter's mixing bound carried through the filter plus gamma_ntaps sum |h| |z|)."""
    M, D, ntaps = 8, 4, 65
    k = np.arange(ntaps) - (ntaps - 1) / 2
    taps = (np.sinc(k / M) * np.hamming(ntaps) / M).astype(F32)
    x = signal(5, 1500)
    y32, _ = PM.channelize32(taps, M, D, x)
    _, S, w_norm = PM.channelize64(taps, M, D, x)
    own = PM.bound(M, ntaps, S, w_norm)
    gamma = ntaps * DM.U / (1.0 - ntaps * DM.U)
    worst = 0.0
    for c in range(M):
        exact, mix_bound = DM.ddc64(taps, D, x, -2.0 * np.pi * c / M)
        err = np.abs(y32[c].astype(np.complex128) - exact)
        ratio = float((err / (own + math.sqrt(2.0) * (mix_bound + gamma * S))).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (c, ratio)
        assert np.abs(exact).max() > 100 * err.max()  # (the agreement is not that of two small numbers)
    print(f"against the down-converter's float64 model: worst error / bound {worst:.4f}")


# ------------------------------------------------------------------ small checks
def test_counts_geometry_and_tile():
    for D in (1, 3, 4, 255, 256):
        for position in (0, 1, D - 1, D, 987654321, PM.MAX_POSITION):
            for n_in in (0, 1, D - 1, D, 1000, PM.MAX_SAMPLES):
                assert pfbch_produce(position, D, n_in) == DM.produce(position, D, n_in) == PM.produce(position, D, n_in)
    for M, D, ntaps in ((2, 1, 1), (2, 2, 4096), (8, 3, 40), (256, 256, 4096), (256, 1, 1), (64, 32, 1025), (16, 8, 257), (32, 31, 33)):
        assert pfbch_geometry(M, D, ntaps) == PM.geometry(M, D, ntaps)
        assert pfbch_tile(M, D, ntaps) == PM.tile(M, D, ntaps) >= 4
        assert (PM.tile(M, D, ntaps) - 1) * D + ntaps - 1 + M <= PM.SPAN


def test_a_scrambled_selection_picks_those_rows():
    M, D, ntaps = 8, 3, 19
    taps, x = random_taps(1, ntaps), signal(2, 300)
    full, _ = PM.channelize32(taps, M, D, x)
    sel = [6, 1, 7, 0]
    picked, _ = PM.channelize32(taps, M, D, x, channels=sel)
    assert picked.shape == (4, full.shape[1]) and np.array_equal(PM.bits(picked), PM.bits(full[sel]))


def test_the_twiddles_are_the_spectrum_stage_s():
    for M in (64, 128, 256):
        assert np.array_equal(PM.bits(pfbch_twiddles(M)), PM.bits(spectrum_twiddles(M)))
    for M in (2, 4, 8, 16, 32, 64, 128, 256):
        got = pfbch_twiddles(M)
        assert got.dtype == np.complex64 and got.shape == (M // 2,) and np.array_equal(got, SM.twiddles64(M).astype(np.complex64))
    with pytest.raises(Exception):
        pfbch_twiddles(3)
    with pytest.raises(Exception):
        pfbch_twiddles(512)


# ------------------------------------------------------------------ special values
def test_special_values_are_the_float32_operations_own():
    """An infinite and a NaN sample make every channel of exactly the outputs whose taps reach them non-finite and leave every other output
    the bits it has without them; denormals are kept; a branch sum starts at +0.0, so -0.0 in gives +0.0 out."""
    M, D, ntaps = 8, 3, 11
    taps, x = random_taps(3, ntaps), signal(4, 400)
    clean, _ = PM.channelize32(taps, M, D, x)
    bad = x.copy()
    bad[100] = np.complex64(complex(np.inf, 1.0))
    bad[250] = np.complex64(complex(2.0, np.nan))
    got, _ = PM.channelize32(taps, M, D, bad)
    k = np.arange(got.shape[1]) * D
    reached = ((k >= 100) & (k - ntaps < 100)) | ((k >= 250) & (k - ntaps < 250))
    assert reached.sum() >= 6
    assert (~np.isfinite(got[:, reached])).any(axis=0).all()
    assert np.array_equal(PM.bits(got[:, ~reached]), PM.bits(clean[:, ~reached]))
    # one tap of 1.0: the branch sum of residue (k D) mod M is +0.0 + x[k D], the others +0.0; the transform of one non-zero point
    tiny = np.zeros(16, np.complex64)
    tiny[4] = np.complex64(complex(1e-41, -1e-41))
    tiny[8] = np.complex64(complex(-0.0, -0.0))
    y, _ = PM.channelize32(np.ones(1, F32), 4, 4, tiny)
    assert y.shape == (4, 4)
    assert (y[:, 1].real == F32(1e-41)).all() and (y[:, 1].imag == F32(-1e-41)).all() and F32(1e-41) != 0  # residue 0: every channel the sample
    assert (PM.bits(y[:, 2]) == 0).all() and (PM.bits(y[:, 0]) == 0).all()  # +0.0, not -0.0


# ------------------------------------------------------------------ the timing tool's torch route
def test_the_timing_tool_s_torch_route_computes_the_channelizer():
    """tools/pfbch_time.py compares the stage with a torch route; that route is held here, on the CPU and a short input, against the
    float64 model, so that the comparison is one of equals (float32 arithmetic in another order: a relative 1e-5 of the largest output)."""
    import torch
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "pfbch_time.py")
    spec = importlib.util.spec_from_file_location("pfbch_time", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for M, sel in ((8, [6, 1]), (16, list(range(16)))):
        D, ntaps = M // 2, 16 * M + 1
        taps, x = tool.lowpass(M, ntaps), signal(M, 50 * M)
        got = tool.make_torch_route(torch.from_numpy(x), taps, M, D, sel)().numpy()
        want, _, _ = PM.channelize64(taps, M, D, x)
        assert got.shape == (len(sel), x.size // D)
        assert np.abs(got - want[sel]).max() <= 1e-5 * np.abs(want).max()
