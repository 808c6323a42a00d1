"""A create that passes the entry's own checks and fails inside the stage class: code, text, no handle, and nothing left behind.

The create entries check the device before they construct the stage class (hence the gpu mark), and most of them check their arguments
first, so only some constructor texts can be reached through the C ABI without a device failure. These are the ones that travel through
make_handle, which turns what the constructor recorded into the code of the C ABI:
  - ldpc (dvbs2_ldpc_create_table): message length, max_frames and group_size are the class's checks;
  - bch (dvbs2_bch_create_raw): the class builds the code and checks n, k and max_frames;
  - demap, plpayload, bbdeheader (raw): the entry checks nothing, every argument text is the class's;
  - plframe: the entry checks plsc and gold code, max_frames is refused by the PlPayloadHip the class owns and forwarded;
  - chain: the texts of its demapper and LDPC stages come through unchanged (its BCH stage refuses nothing the two before it accept).
plsync, plcoarse, rotator and symsync have no such case: their entries make every check of the constructor first (dvbs2_symsync_create_taps
runs the same SymSyncHip::check_args as the class), so their constructors fail on a device failure only.
Each case asserts the code, the full text of dvbs2_last_error() and that *h is null, then creates a good handle of the same type at its
smallest legal size and makes one good call whose outputs equal those of a handle created before any failure -- nothing of the failed
create stays in the thread's state but the text of the last error, which a call that succeeds does not clear.
The codes and texts were recorded from the library before the stage classes carried a code with their text."""
import ctypes as C

import pytest

import fec_testlib as T
import plsync_model as P
from dvbs2rx_amd import capi, rate_id
from dvbs2rx_amd.capi import lib
from test_stage_call_errors_gpu import MF, QPSK, SHORT, STAGES, TABLE, reference

pytestmark = pytest.mark.gpu

EINVAL, OK, S2 = capi.EINVAL, capi.OK, capi.STANDARD_DVBS2
K = T.ldpc_info(TABLE)[1]
BCH = (14, 0x402B, 12, 3240)  # m, primitive polynomial, t, n of the short frames' outer code at rate 1/4

FRAMES_DIM = "max_frames must be in 1..65535 (frames are one launch dimension)"
LDPC_SIZES = "bad group_size/max_frames (max_frames 1..65535: frames are one launch dimension)"
APSK_RATE = "Unsupported code rate for 16APSK / 32APSK (DVB-S2: 16APSK 2/3 .. 9/10, 32APSK 3/4 .. 9/10; 9/10 normal frames only)"


def c1_4():
    return rate_id("C1_4")


CASES = [  # (handle type, what the class refuses, create(h) -> code, expected code, expected text)
    ("ldpc", "message_bits", lambda h: lib.dvbs2_ldpc_create_table(h, TABLE.encode(), K - 4, 2, MF, 0), EINVAL, "bad message length"),
    ("ldpc", "max_frames", lambda h: lib.dvbs2_ldpc_create_table(h, TABLE.encode(), K, 2, 65536, 0), EINVAL, LDPC_SIZES),
    ("ldpc", "group_size", lambda h: lib.dvbs2_ldpc_create_table(h, TABLE.encode(), K, 0, MF, 0), EINVAL, LDPC_SIZES),
    ("bch", "n", lambda h: lib.dvbs2_bch_create_raw(h, BCH[0], BCH[1], BCH[2], BCH[3] - 4, MF, 0), EINVAL,
     "u8 array messages are only supported for n and k multiple of 8."),
    ("bch", "max_frames", lambda h: lib.dvbs2_bch_create_raw(h, *BCH, 0, 0), EINVAL, FRAMES_DIM),
    ("demap", "constellation", lambda h: lib.dvbs2_demap_create(h, SHORT, c1_4(), 2, MF, 0), EINVAL, "Unsupported constellation"),
    ("demap", "apsk_rate", lambda h: lib.dvbs2_demap_create(h, SHORT, c1_4(), capi.MOD_16APSK, MF, 0), EINVAL, APSK_RATE),
    ("plpayload", "gold_code", lambda h: lib.dvbs2_plpayload_create(h, (1 << 18) - 1, 36, 1, MF, 0), EINVAL, "gold code out of range"),
    ("plpayload", "n_slots", lambda h: lib.dvbs2_plpayload_create(h, 0, 35, 1, MF, 0), EINVAL, "n_slots out of range (36..360)"),
    ("plframe", "max_frames", lambda h: lib.dvbs2_plframe_create(h, 0, P.SHORT_QPSK, 0, 0), EINVAL, FRAMES_DIM),
    ("bbdeheader", "kbch_bits", lambda h: lib.dvbs2_bbdeheader_create_raw(h, 84, MF, 0), EINVAL, "unsupported BCH message length"),
    ("bbdeheader", "max_frames", lambda h: lib.dvbs2_bbdeheader_create_raw(h, 3072, 0, 0), EINVAL, "max_frames must be in 1..65535"),
    ("chain", "demap_stage", lambda h: lib.dvbs2_chain_create(h, S2, SHORT, c1_4(), 2, 2, MF, 0), EINVAL, "Unsupported constellation"),
    ("chain", "ldpc_stage", lambda h: lib.dvbs2_chain_create(h, S2, SHORT, c1_4(), QPSK, 0, MF, 0), EINVAL, LDPC_SIZES),
]


def test_the_handle_types_with_a_reachable_constructor_text():
    assert {c[0] for c in CASES} == set(STAGES) - {"plsync", "plcoarse", "rotator", "symsync"}


@pytest.mark.parametrize("stage,what,create,code,text", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_failed_create_gives_code_text_and_no_handle(stage, what, create, code, text):
    make, good = STAGES[stage]
    want = reference(stage)
    h = C.c_void_p(0x5a5a5a58)  # never dereferenced: the entry writes null before anything else
    rc = create(C.byref(h))
    got_text = lib.dvbs2_last_error().decode()
    print(f"{stage}-{what}: code {rc} text {got_text!r} handle {h.value}")
    assert (rc, got_text) == (code, text)
    assert h.value is None
    o = make()
    assert good(o) == want, "after the failed create a new handle answers differently from one created before it"
    assert lib.dvbs2_last_error().decode() == text  # the last ERROR: a create and a call that succeed do not clear it
    o.close()
