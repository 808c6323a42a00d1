"""The closed loop the stream-stage tests share, noise-free unless the test adds noise: FecEncoder -> PlFramer behind a random lead ->
(a test's own stages) -> SymbolSync -> PlSync -> gather -> PlCoarse -> PlFrontEnd -> FecChain -> the encoder's input bytes. Each piece is
a function with explicit arguments; a test puts the stage it is about between them and keeps the checks that are its own.
notes/test_harness.md says how a new stage's test uses them."""
import collections

import numpy as np

import fec_testlib as T
import plframe_model as M
import plsync_model as P
from dvbs2rx_amd import (FecChain, FecEncoder, PlCoarse, PlFramer, PlFrontEnd, PlSync, SymbolSync, capi, plframer_layout, pulse_taps,
                         symsync_taps)

QPSK_1_4_SHORT = dict(standard=capi.STANDARD_DVBS2, framesize=capi.FECFRAME_SHORT, rate="C1_4", constellation=capi.MOD_QPSK)
DUMMY = P.plsc_of(0, 0, 0)


def transmit_symbols(seq, nd, gold, lead, seed, flush, fec=QPSK_1_4_SHORT):
    """nd scrambled frames of random bytes through the encoder, then the PL framer over the PLSC sequence seq (its nd data frames and
    any dummy frames) behind `lead` random QPSK symbols. From one generator of `seed`: the bytes first, then the lead. Returns (the
    encoder's input bytes [nd, in_bytes], the symbols on the device as float32 [n_all, 2]: lead, frames, the 90 symbols of the closing
    header and `flush` zero symbols, n without the flush, n_all, the framer's layout)."""
    import torch
    rng = np.random.default_rng(seed)
    st = T.stream()
    enc = FecEncoder(max_frames=nd, **fec)
    enc.set_scramble(True)
    sent = rng.integers(0, 256, (nd, enc.in_bytes), dtype=np.uint8)
    lay = plframer_layout(seq)
    assert lay["in_syms"] == nd * enc.n_syms and all(M.pls_parse(q)["xfecframe_len"] == enc.n_syms for q in seq if q != DUMMY)
    d_xfec = torch.zeros((nd, enc.n_syms, 2), dtype=torch.float32, device="cuda")
    enc.work_device(torch.from_numpy(sent).cuda().data_ptr(), nd, d_syms=d_xfec.data_ptr(), stream=st)
    fr = PlFramer(gold, max_frames=len(seq))
    fr.set_sequence(seq)
    n = lead + lay["out_syms"] + 90
    n_all = n + flush
    d_x = torch.zeros((n_all, 2), dtype=torch.float32, device="cuda")
    d_x[:lead] = torch.from_numpy(P.qpsk(rng, lead).astype(np.complex64).view(np.float32).reshape(-1, 2)).cuda()
    fr.work_device(d_xfec.data_ptr(), len(seq), seq[-1], d_x.data_ptr() + 8 * lead, st)
    torch.cuda.synchronize()
    fr.close()
    enc.close()
    return sent, d_x, n, n_all, lay


def unit_amplitude_taps(sps, rolloff, rrc_delay, tau=0.0):
    """The pulse shaper's design shifted by tau symbols, scaled so that the centre of the convolution of the UNSHIFTED design with
    subfilter 0 of the receiver's bank (its matched filter at mu = 0) is 1: unit symbol amplitude behind the matched filter at the right
    instant. The shift moves the pulse and leaves its scale alone."""
    bank0 = symsync_taps(sps, rolloff, rrc_delay, 128)[0].astype(np.float64)[::-1]  # the bank holds each subfilter flipped
    centre = np.convolve(pulse_taps(sps, rolloff, rrc_delay).astype(np.float64), bank0)[2 * sps * rrc_delay]
    return (pulse_taps(sps, rolloff, rrc_delay, tau).astype(np.float64) / centre).astype(np.float32)


GOLD, PLSC = 5, P.plsc_of(1, 1, 1)
SEQ6 = [PLSC, PLSC, DUMMY, PLSC, PLSC, DUMMY, PLSC, PLSC]  # six short QPSK 1/4 frames with pilots, a dummy frame after data frames 2 and 4
SPS, ROLLOFF, RRC_DELAY, TAU = 2, 0.2, 5, 0.3

Shaped = collections.namedtuple("Shaped", "sent d_y ns n_all lay lead")


def shaped_six_frames(lead, seed):
    """transmit_symbols(SEQ6) through the pulse shaper at SPS samples per symbol with a timing offset of TAU symbols, the taps through
    create_taps and scaled by unit_amplitude_taps; the flush is the shaper's history and 64 symbols more. Returns Shaped: the encoder's
    input, the samples on the device as float32 [ns, 2], ns, the number of symbols with the flush, the framer's layout and the lead."""
    import torch
    from dvbs2rx_amd import PulseShaper, pulse_geometry
    history = pulse_geometry(SPS, RRC_DELAY)[1]
    sent, d_x, n, n_all, lay = transmit_symbols(SEQ6, 6, GOLD, lead, seed, flush=history + 64)
    ps = PulseShaper(SPS, taps=unit_amplitude_taps(SPS, ROLLOFF, RRC_DELAY, TAU), max_symbols=n_all)
    assert ps.history == history
    d_y = torch.zeros((n_all * SPS, 2), dtype=torch.float32, device="cuda")
    ps.work_device(d_x.data_ptr(), n_all, n_all, 1, d_y.data_ptr(), n_all * SPS, T.stream())
    torch.cuda.synchronize()
    ps.close()
    return Shaped(sent, d_y, n_all * SPS, n_all, lay, lead)


Frames = collections.namedtuple("Frames", "recs d_sym d_rec nf sync state nsym loop")


def timing_and_frames(d_y, ns, sps, rolloff, interp_method, n_syms, tol, plsc=-1):
    """d_y: ns samples at sps per symbol on the device. SymbolSync (loop bandwidth 0.01, damping 1), then PlSync(plsc) on its symbols.
    Requires the loop's status 0 and its symbol count within tol of n_syms. Returns Frames: the frame records, the symbols and all
    records on the device, the number of records, the PlSync (open: the caller closes it), the tracker's state, the number of symbols
    and the loop's final state."""
    import torch
    st = T.stream()
    ss = SymbolSync(sps=sps, loop_bw=0.01, damping=1.0, rolloff=rolloff, interp_method=interp_method, max_samples=ns)
    d_sym = torch.zeros(2 * ns, dtype=torch.float32, device="cuda")
    ss.work_device(d_y.data_ptr(), ns, [ns], d_sym.data_ptr(), ns, ns, 0, 0, st)
    n_out, _, status = ss.finish()
    nsym, loop = int(n_out[0]), ss.state()
    ss.close()
    assert status[0] == 0 and abs(nsym - n_syms) <= tol, (status[0], nsym, n_syms, tol)
    sync = PlSync(plsc=plsc, max_symbols=max(nsym, PlSync.MIN_SYMBOLS), max_frames=64)
    d_rec = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
    sync.work_device(d_sym.data_ptr(), nsym, d_rec.data_ptr(), st)
    nf, _, state = sync.finish()
    recs = d_rec.cpu().numpy().view(PlSync.FRAME_DTYPE)[:nf]
    return Frames(recs, d_sym, d_rec, nf, sync, state, nsym, loop)


Decoded = collections.namedtuple("Decoded", "msg data_index locked offsets corrected")


def decode_frames(rx, plsc, gold, n0, fec=QPSK_1_4_SHORT, descramble=True, first_sof=0):
    """The decode tail on the Frames rx: gather the locked frames of `plsc`, coarse estimate, front end, FEC chain at noise power n0.
    The locked records with a SOF below first_sof (a lead in which an AGC still settles) are not expected: every gathered frame must lie
    at or behind it. Requires the gathered count to be the number of those records, and every frame out of the LDPC and BCH decoders
    without a failure. Returns Decoded: the messages, which data frame at or behind first_sof each carries, the records' indices, the
    coarse estimates and the coarse_corrected flags."""
    import torch
    st = T.stream()
    recs = rx.recs
    L = M.pls_parse(plsc)["plframe_len"]
    locked = [f for f, r in enumerate(recs) if r["flags"] & capi.PLSYNC_FLAG_LOCKED and r["plsc"] == plsc and r["sof_index"] >= first_sof]
    d_fr = torch.zeros((len(locked) * L + 90) * 2, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rx.sync.gather_device(rx.d_sym.data_ptr(), rx.d_rec.data_ptr(), rx.nf, plsc, d_fr.data_ptr(), d_cnt.data_ptr(), st)
    torch.cuda.synchronize()
    cnt = int(d_cnt.item())
    assert cnt == len(locked), (cnt, locked)
    pc = PlCoarse(1, plsc, max_frames=64)
    d_cc = torch.zeros(cnt, dtype=torch.int32, device="cuda")
    d_f = torch.zeros(cnt, dtype=torch.float32, device="cuda")
    pc.work_device(d_fr.data_ptr(), L, cnt, 0, d_f.data_ptr(), d_cc.data_ptr(), 0, st)
    fe = PlFrontEnd(gold, plsc, max_frames=cnt)
    d_rx = torch.zeros((cnt, fe.xfecframe_len * 2), dtype=torch.float32, device="cuda")
    fe.work_device(d_fr.data_ptr(), cnt, 1, d_cc.data_ptr(), d_f.data_ptr(), d_rx.data_ptr(), st)
    torch.cuda.synchronize()
    chain = FecChain(group_size=4, max_frames=cnt, max_trials=25, **fec)
    if descramble:
        chain.set_descramble(True)
    msg, ret, corr = chain.work(d_rx.cpu().numpy().view(np.complex64), np.float32(n0))
    for o in (chain, fe, pc):
        o.close()
    assert (ret >= 0).all() and (corr >= 0).all(), (ret, corr)
    first = int(np.nonzero(recs["sof_index"] >= first_sof)[0][0])
    data_index = [int(np.count_nonzero(recs["plsc"][first:f] == plsc)) for f in locked]  # which data frame each gathered frame carries
    return Decoded(msg, data_index, locked, d_f.cpu().numpy(), d_cc.cpu().numpy())
