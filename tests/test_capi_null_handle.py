"""Every entry of the C ABI that takes a handle answers a null one without touching it.

The expected answers were recorded from the library as it was before the C-ABI layer was split by stage (notes/capi_split.md): every
entry returned what is listed here, none of them crashed. Needs no GPU: the null check comes before anything that uses a device."""
import ctypes as C

from dvbs2rx_amd import capi

HANDLE_TYPES = ("ldpc", "bch", "demap", "chain", "plpayload", "plframe", "plsync", "plcoarse", "rotator", "symsync", "bbdeheader")
HOST_ONLY = {"dvbs2_plsync_taps", "dvbs2_plsync_thresholds"}  # first argument is an output buffer, not a handle
# the getters that do not return a status: their documented answer for a null handle
NULL_ANSWER = {"dvbs2_ldpc_kernel_name": None, "dvbs2_chain_ldpc_kernel_name": None,
               "dvbs2_ldpc_fallback_rounds": -1, "dvbs2_chain_ldpc_fallback_rounds": -1}
# the two entries that check their handle and their output structure in one test
NULL_TEXT = {"dvbs2_symsync_state": b"bad argument", "dvbs2_bbdeheader_counters": b"bad argument"}


def _handle_entries():
    for name, (_, args) in capi.SYMBOLS.items():
        if name.split("_")[1] in HANDLE_TYPES and args and args[0] is C.c_void_p and name not in HOST_ONLY and "_create" not in name:
            yield name


def test_null_handle():
    names = list(_handle_entries())
    assert len(names) == 85 and all(f"dvbs2_{t}_destroy" in names for t in HANDLE_TYPES)
    wrong = []
    for name in names:
        zero = [0 if a in (C.c_int, C.c_int64, C.c_double, C.c_float, C.c_uint32, C.c_size_t) else None for a in capi.SYMBOLS[name][1]]
        assert capi.lib.dvbs2_get_fec_info(0, 0, 0, None) == capi.EINVAL  # leaves "null out" behind: the text below is this entry's own
        ret = getattr(capi.lib, name)(*zero)
        if name.endswith("_destroy"):
            got, want = ret, None  # void: a null handle is ignored
        elif name in NULL_ANSWER:
            got, want = ret, NULL_ANSWER[name]
        else:
            got, want = (ret, capi.lib.dvbs2_last_error()), (capi.EINVAL, NULL_TEXT.get(name, b"null handle"))
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, wrong
