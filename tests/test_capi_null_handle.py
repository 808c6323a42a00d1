"""The census of the whole C ABI: every entry that takes a handle answers a null one without touching it, and every create answers a null
handle pointer in front of its argument checks.

Which entries those are is read from include/dvbs2_fec_hip.h by the rule of T.c_abi_declarations (notes/capi_census.md): a new entry joins
by being declared. The numbers below were found on the library as it was when the rule replaced the frozen lists; the exceptions were
recorded from the library as it was before the C-ABI layer was split by stage (notes/capi_split.md). Needs no GPU: the null check comes
before anything that uses a device."""
import collections

import fec_testlib as T
from dvbs2rx_amd import capi

# handle entries per handle type (25 types, 184 entries)
ENTRIES = {"ldpc": 9, "bch": 6, "demap": 9, "chain": 14, "enc": 5, "plframer": 5, "plpayload": 4, "plframe": 10, "plsync": 9, "plcoarse": 5,
           "awgn": 6, "iqconv": 7, "agc": 9, "rotator": 8, "symsync": 7, "pulse": 5, "plsync_batch": 8, "resamp": 10, "ddc": 9, "spectrum": 4,
           "pfbch": 8, "pfbsyn": 8, "bbdeheader": 7, "bbframer": 8, "plcoarse_batch": 4}
# the getters that do not return a status: their documented answer for a null handle
NULL_ANSWER = {"dvbs2_ldpc_kernel_name": None, "dvbs2_chain_ldpc_kernel_name": None,
               "dvbs2_ldpc_fallback_rounds": -1, "dvbs2_chain_ldpc_fallback_rounds": -1}
# the two entries that check their handle and their output structure in one test
NULL_TEXT = {"dvbs2_symsync_state": b"bad argument", "dvbs2_bbdeheader_counters": b"bad argument"}
# the create that checks another argument in front of its handle pointer (recorded, not changed)
CREATE_TEXT = {"dvbs2_symsync_create_taps": b"null bank"}


def test_null_handle():
    decls = T.c_abi_declarations()
    handles = [d for d in decls if d.kind == "handle"]
    creates = [d.name for d in decls if d.kind == "create"]
    per_type = collections.Counter(d.type for d in handles)
    assert len(per_type) == 25 and len(handles) == 184 and len(creates) == 36
    assert per_type == ENTRIES, {t: (per_type.get(t), ENTRIES.get(t)) for t in set(per_type) | set(ENTRIES) if per_type.get(t) != ENTRIES.get(t)}
    assert all(f"dvbs2_{t}_destroy" in {d.name for d in handles if d.type == t} for t in ENTRIES)
    wrong = []
    for name in [d.name for d in handles] + creates:
        assert capi.lib.dvbs2_get_fec_info(0, 0, 0, None) == capi.EINVAL  # leaves "null out" behind: the text below is this entry's own
        ret = getattr(capi.lib, name)(*T.c_zero_args(capi.SYMBOLS[name][1]))
        if name in creates:
            got, want = (ret, capi.lib.dvbs2_last_error()), (capi.EINVAL, CREATE_TEXT.get(name, b"null handle pointer"))
        elif name.endswith("_destroy"):
            got, want = ret, None  # void: a null handle is ignored
        elif name in NULL_ANSWER:
            got, want = ret, NULL_ANSWER[name]
        else:
            got, want = (ret, capi.lib.dvbs2_last_error()), (capi.EINVAL, NULL_TEXT.get(name, b"null handle"))
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, wrong
