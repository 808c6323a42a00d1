#!/usr/bin/env python3
"""tools/gen_live_golden.py -- BUILD CONTAINER ONLY. What the genuine reference (oracle/_ref) answers to the seeded inputs of the three
"live" CPU tests -> tests/golden/ref_live_golden.json, so that those tests check the restatement against the reference's answers
where oracle/_ref cannot be built (and, where it can, against both):
  crc8  tests/test_bbdeheader.py::test_crc8_oracle_vs_reference_live   ref_crc8_rem of 2000 random strings (lib/gf_util.h)
  ldpc  tests/test_oracle_kat.py::test_ldpc_oracle_vs_reference_live   AVX2 decoder, S2_TABLE_C3, 32 AWGN frames, 20 iterations
  bch   tests/test_oracle_kat.py::test_bch_oracle_vs_reference_live    bch_codec encode + decode of 12 words per code (lib/bch.cc)
The inputs are drawn exactly as the tests draw them."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fec_testlib as T

assert T.ref_ldpc() is not None and T.ref_bch() is not None, "run `make -C oracle` in the build container first"
out = {"source": "genuine reference through oracle/_ref (tools/gen_live_golden.py)"}

ref = T.ref_bch()
rng = np.random.default_rng(11)
rem = []
for _ in range(2000):
    n = int(rng.integers(1, 400))
    d = rng.integers(0, 256, n, dtype=np.uint8)
    rem.append(int(ref.ref_crc8_rem(T.ptr(d), n)))
out["crc8_rem"] = rem

x = T.make_input("S2_TABLE_C3", "awgn", 32, seed=21, amp=5, sigma=5.5)
b, rb = T.ref_ldpc_decode("S2_TABLE_C3", x, 0, 20)
out["ldpc_c3"] = {"ret": [int(v) for v in rb], "llr_sha256": T.sha(b)}

rng = np.random.default_rng(99)
out["bch"] = []
for fs, n, t in ((0, 3240, 12), (1, 32400, 12), (1, 58320, 8)):
    m, prim = T.BCH_FIELDS[fs]
    rb_ = T.RefBch(prim, t, n)
    msg = rng.integers(0, 256, (12, T.OracleBch(m, prim, t, n).k // 8), dtype=np.uint8)
    cw = rb_.encode(msg)
    rx = np.stack([T.flip_bits(cw[i], rng.choice(n, [0, 1, 2, t, t + 1, 15, 20, 30, 40, 41, 42, 100][i], replace=False)) for i in range(12)])
    want, wret = rb_.decode(rx)
    out["bch"].append({"fs": fs, "n": n, "t": t, "cw_sha256": T.sha(np.asarray(cw, np.uint8)),
                       "msg_sha256": T.sha(np.asarray(want, np.uint8)), "ret": [int(v) for v in wret]})
    rb_.close()
json.dump(out, open(os.path.join(ROOT, "tests", "golden", "ref_live_golden.json"), "w"), indent=0)
print("crc8", len(rem), "ldpc ret", out["ldpc_c3"]["ret"], "bch", [e["ret"] for e in out["bch"]])
