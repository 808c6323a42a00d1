"""Shared helpers for the tests: loads the CPU checkers (oracle/) and builds deterministic inputs.

Only test code (tests/, __graft_entry__.smoke(), bench.py's cpu_baseline leg) may import this
module: it is the bridge to oracle/ and is never used by the product path.
"""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")


def _build_oracle():
    so = os.path.join(ORACLE_DIR, "liboracle.so")
    srcs = [os.path.join(ORACLE_DIR, f) for f in ("ldpc_oracle.c", "bch_oracle.c", "demap_oracle.c", "bb_oracle.c", "bbdeheader_oracle.c", "pl_oracle.c")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "liboracle.so"], stdout=subprocess.DEVNULL)
    return so


_oracle = None


def oracle():
    """ctypes handle of oracle/liboracle.so (the plain-C restatement)."""
    global _oracle
    if _oracle is None:
        o = C.CDLL(_build_oracle())
        o.oracle_ldpc_decode.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int]
        o.oracle_ldpc_decode.restype = C.c_int
        o.oracle_ldpc_pack.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        o.oracle_ldpc_encode.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
        o.oracle_ldpc_info.argtypes = [C.c_char_p] + [C.POINTER(C.c_int)] * 4
        o.oracle_bch_new.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_int]
        o.oracle_bch_new.restype = C.c_void_p
        o.oracle_bch_free.argtypes = [C.c_void_p]
        for f in ("oracle_bch_k", "oracle_bch_n", "oracle_bch_gdeg"):
            getattr(o, f).argtypes = [C.c_void_p]
        o.oracle_bch_genpoly.argtypes = [C.c_void_p, C.c_void_p]
        o.oracle_bch_alpha.argtypes = [C.c_void_p, C.c_int]
        o.oracle_bch_alpha.restype = C.c_uint32
        o.oracle_bch_minpoly.argtypes = [C.c_void_p, C.c_int]
        o.oracle_bch_minpoly.restype = C.c_uint32
        o.oracle_bch_encode_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        o.oracle_bch_syndrome_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        o.oracle_bch_err_loc_poly.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        o.oracle_bch_err_loc_numbers.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        o.oracle_bch_decode_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        o.oracle_bch_encode_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        o.oracle_demap_qpsk.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        o.oracle_demap_8psk.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p]
        o.oracle_demap_snr.argtypes = [C.c_void_p, C.c_int, C.c_int]
        o.oracle_demap_snr.restype = C.c_float
        o.oracle_demap_snr_refined.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        o.oracle_demap_snr_refined.restype = C.c_float
        o.oracle_bb_sequence.argtypes = [C.c_void_p, C.c_int]
        o.oracle_pl_rn.argtypes = [C.c_int, C.c_void_p, C.c_int]
        o.oracle_pl_payload.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        o.oracle_bb_descramble.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        o.oracle_crc8_rem.argtypes = [C.c_void_p, C.c_int]
        o.oracle_crc8_rem.restype = C.c_uint8
        o.oracle_bbdh_init.argtypes = [C.c_void_p, C.c_int]
        o.oracle_bbdh_work.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        o.oracle_bbdh_work.restype = C.c_longlong
        _oracle = o
    return _oracle


_ref = None


def ref_ldpc():
    """ctypes handle of oracle/_ref/libdvbs2_ref_ldpc.so (the genuine reference LDPC decoders), or None."""
    global _ref
    if _ref is None:
        p = os.path.join(ORACLE_DIR, "_ref", "libdvbs2_ref_ldpc.so")
        if not os.path.exists(p):
            return None
        r = C.CDLL(p)
        r.ref_ldpc_init.argtypes = [C.c_char_p, C.c_int]
        r.ref_ldpc_decode.argtypes = [C.c_void_p, C.c_int]
        _ref = r
    return _ref


_ref_bch = None


def ref_bch():
    """ctypes handle of oracle/_ref/libdvbs2_ref_bch.so (the genuine reference BCH codec), or None."""
    global _ref_bch
    if _ref_bch is None:
        p = os.path.join(ORACLE_DIR, "_ref", "libdvbs2_ref_bch.so")
        if not os.path.exists(p):
            return None
        r = C.CDLL(p)
        r.ref_bch_new.argtypes = [C.c_uint32, C.c_int, C.c_int]
        r.ref_bch_new.restype = C.c_void_p
        r.ref_bch_free.argtypes = [C.c_void_p]
        r.ref_bch_k.argtypes = [C.c_void_p]
        r.ref_bch_n.argtypes = [C.c_void_p]
        r.ref_bch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        r.ref_bch_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        r.ref_crc8_rem.argtypes = [C.c_void_p, C.c_int]
        _ref_bch = r
    return _ref_bch


class RefBch:
    """The genuine reference bch_codec<uint32_t, bitset256_t> (container build, oracle/_ref). decode() returns the
    reference's return value, or -2 where it throws."""

    def __init__(self, prim_poly, t, n=0):
        self.r = ref_bch()
        assert self.r is not None, "oracle/_ref/libdvbs2_ref_bch.so absent"
        self.h = self.r.ref_bch_new(prim_poly, t, n)
        assert self.h, "reference constructor threw"
        self.n, self.k = self.r.ref_bch_n(self.h), self.r.ref_bch_k(self.h)

    def decode(self, cw):
        cw = np.ascontiguousarray(cw, np.uint8).reshape(-1, self.n // 8)
        msg = np.zeros((cw.shape[0], self.k // 8), np.uint8)
        ret = [self.r.ref_bch_decode(self.h, ptr(cw[f]), ptr(msg[f])) for f in range(cw.shape[0])]
        return msg, ret

    def encode(self, msg):
        msg = np.ascontiguousarray(msg, np.uint8).reshape(-1, self.k // 8)
        cw = np.zeros((msg.shape[0], self.n // 8), np.uint8)
        for f in range(msg.shape[0]):
            self.r.ref_bch_encode(self.h, ptr(msg[f]), ptr(cw[f]))
        return cw

    def close(self):
        if self.h:
            self.r.ref_bch_free(self.h)
            self.h = None


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ldpc_info(table):
    n, k, q, lt = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert oracle().oracle_ldpc_info(table.encode(), n, k, q, lt) == 0, table
    return n.value, k.value, q.value, lt.value


def oracle_ldpc_decode(table, llr, G, trials):
    """llr: (n_frames, N) int8, n_frames % G == 0. Returns (decoded llr copy, list of return values per group)."""
    out = np.ascontiguousarray(llr).copy()
    rets = []
    for g in range(0, out.shape[0], G):
        blk = out[g:g + G]
        rets.append(oracle().oracle_ldpc_decode(table.encode(), G, ptr(blk), trials))
    return out, rets


def ref_ldpc_decode(table, llr, impl, trials):
    """Genuine reference. impl 0 = AVX2 (G=32), 1 = SSE4.1 (G=16), 2 = generic (G=16)."""
    r = ref_ldpc()
    G = r.ref_ldpc_init(table.encode(), impl)
    assert G > 0
    out = np.ascontiguousarray(llr).copy()
    rets = []
    for g in range(0, out.shape[0], G):
        blk = out[g:g + G]
        rets.append(r.ref_ldpc_decode(ptr(blk), trials))
    return out, rets


def cpu_ldpc_decode_ragged(table, llr, G, trials):
    """Any number of frames: whole groups of G through the genuine reference when it serves that G (32: AVX2), the trailing partial
    group -- a group of its own, like the HIP path treats it -- through the scalar restatement (which takes any group size)."""
    nf = llr.shape[0]
    full = nf - nf % G
    outs, rets = [], []
    if full:
        if ref_ldpc() is not None and G == 32:
            o, r = ref_ldpc_decode(table, llr[:full], 0, trials)
        else:
            o, r = oracle_ldpc_decode(table, llr[:full], G, trials)
        outs.append(o); rets += list(r)
    if nf > full:
        o, r = oracle_ldpc_decode(table, llr[full:], nf - full, trials)
        outs.append(o); rets += list(r)
    return np.concatenate(outs), rets


def ref_ldpc_decode_parallel(table, llr, impl, trials, procs=None):
    """Genuine reference on a WHOLE batch: worker processes (tools/cpu_ref_decode_worker.py), each decoding a contiguous
    range of groups of a shared .npy file in /dev/shm. Returns (decoded llr, list of return values per group), identical
    to ref_ldpc_decode(). n_frames must be a multiple of the reference's batch (32 for AVX2, 16 otherwise)."""
    import sys
    import tempfile
    G = 32 if impl == 0 else 16
    nf = llr.shape[0]
    assert nf % G == 0, "whole reference batches only"
    ng = nf // G
    if procs is None:
        procs = max(1, min(len(os.sched_getaffinity(0)), 64, ng))
    if procs == 1 or ng < 4:
        return ref_ldpc_decode(table, llr, impl, trials)
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        f_llr, f_ret = os.path.join(d, "llr.npy"), os.path.join(d, "ret.npy")
        np.save(f_llr, np.ascontiguousarray(llr, np.int8))
        np.save(f_ret, np.zeros(ng, np.int32))
        worker = os.path.join(ROOT, "tools", "cpu_ref_decode_worker.py")
        cuts = [ng * i // procs for i in range(procs + 1)]
        ps = [subprocess.Popen([sys.executable, worker, table, str(impl), str(trials), f_llr, f_ret, str(cuts[i]), str(cuts[i + 1])])
              for i in range(procs) if cuts[i + 1] > cuts[i]]
        for p in ps:
            assert p.wait() == 0, "reference worker failed"
        return np.load(f_llr), np.load(f_ret).tolist()


def pack_bits(llr, nbits):
    """Hard decision + MSB-first packing (lib/ldpc_decoder_bb_impl.cc:432-442)."""
    out = np.zeros((llr.shape[0], nbits // 8), np.uint8)
    oracle().oracle_ldpc_pack(ptr(np.ascontiguousarray(llr)), llr.shape[0], llr.shape[1], nbits, ptr(out))
    return out


# ------------------------------------------------------------------ kernel builds
VARIANTS = {  # every build of the sweep kernel gives the same bits (environment overrides of the per-table policy)
    "policy": {},
    "pr-byte-records": {"DVBS2_PR_W1": "0"},                                                       # parity in records with two-dword records also for degree <= 4
    "pr-plain": {"DVBS2_PR_V2": "0"},                                                             # the two-dword-record kernel with its plain nodes everywhere
    "pr-packed": {"DVBS2_PR": "1", "DVBS2_PR_W1": "0", "DVBS2_PR_V2": "1"},                          # parity in records on every eligible table (normal frames too), packed nodes in the regular middle layers
    "classic": {"DVBS2_PR": "0", "DVBS2_DENSE": "0"},                                              # no parity-in-records / dense build
    "plain": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "0", "DVBS2_SOLO": "0"},          # byte messages, scalar nodes, pair workgroups
    "packed-pair": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "0"},    # packed nodes, six-bit messages, pair workgroups
    "plain-solo": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "0", "DVBS2_SOLO": "1"},     # scalar nodes, one frame per workgroup
    "packed-solo": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "1"},
    "packed-pair-plain-hazard": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "0", "DVBS2_V2P": "0"},  # hazard layers through the plain node (what a wave whose record does not fit the packed format runs)
    "heavy-hazard": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "1"},                       # twelve ordered entries, two-level walk (degree classes >= 12)
    "soft-barrier": {"DVBS2_PR": "0", "DVBS2_DENSE": "0", "DVBS2_HZ2": "0", "DVBS2_V2": "1", "DVBS2_SOLO": "0", "DVBS2_SOFT_BARRIER": "1"},  # per-frame software barriers
}


def build_ldpc_planner(out_dir, main=None):
    """The host-only LDPC planner (csrc/ldpc_plan.cpp) behind tests/ldpc_plan_main.cpp, compiled with the host compiler alone."""
    csrc = os.path.join(ROOT, "gr-dvbs2rx_amd", "csrc")
    exe = os.path.join(str(out_dir), "ldpc_plan_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", main or os.path.join(ROOT, "tests", "ldpc_plan_main.cpp")] +
                          [os.path.join(csrc, f) for f in ("ldpc_plan.cpp", "ldpc_schedule.cpp", "fec_tables.cpp")] + ["-o", exe])
    return exe


def build_host_program(tmp_dir, main_cpp, sources, fp_contract_off=True):
    """tests/<main_cpp> with the csrc/ sources it calls, as a stand-alone program in tmp_dir: host code under AddressSanitizer and UBSan
    (device code is not instrumented and none of it runs). Returns the program's path."""
    csrc = os.path.join(ROOT, "gr-dvbs2rx_amd", "csrc")
    exe = os.path.join(str(tmp_dir), os.path.splitext(main_cpp)[0])
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *(["-ffp-contract=off"] if fp_contract_off else []),
                           *san, os.path.join(ROOT, "tests", main_cpp), *[os.path.join(csrc, s) for s in sources], "-o", exe])
    return exe


def run_host_program(exe, rows):
    """One of the stand-alone host programs (build_host_program) with `rows` on its standard input, one per line: the stripped lines of
    its standard output."""
    r = subprocess.run([exe], input="".join(row + "\n" for row in rows), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report goes to stderr and ends the program
    return [line.strip() for line in r.stdout.splitlines()]


# ------------------------------------------------------------------ the C ABI as the public header declares it (notes/capi_census.md)
def c_abi_declarations():
    """Every function include/dvbs2_fec_hip.h declares, by one rule: comments stripped, declarations matched by `name ( params ) ;`, the
    first parameter decides the class. One record per function, in header order: name, ret (the text of the return type), params (the
    parameter texts, [] for `void`), kind and type. The handle types are those with a dvbs2_<type>_destroy; kind is "handle" where the
    first parameter is `[const] dvbs2_<type>_t*` of a handle type (type names it), "create" where it is `dvbs2_<type>_t**`, else "other"."""
    from types import SimpleNamespace as NS
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(ROOT, "include", "dvbs2_fec_hip.h")).read(), flags=re.S)
    found = re.findall(r"\b((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(dvbs2_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)
    types = {name[len("dvbs2_"):-len("_destroy")] for _, name, _ in found if name.endswith("_destroy")}
    decls = []
    for ret, name, params in found:
        params = [" ".join(p.split()) for p in params.split(",")]
        d = NS(name=name, ret="".join(ret.split()).replace("const", "const "), params=[] if params == ["void"] else params, kind="other", type=None)
        first = re.fullmatch(r"(?:const )?dvbs2_([a-z0-9_]+)_t ?(\*\*?) ?\w+", d.params[0]) if d.params else None
        if first and first.group(2) == "**":
            d.kind, d.type = "create", first.group(1)
        elif first and first.group(1) in types:
            d.kind, d.type = "handle", first.group(1)
        decls.append(d)
    return decls


def c_kind_of_text(text):
    """the kind of a parameter or return type as the header spells it: "pointer" (an array parameter such as `uint8_t out[10]` is one),
    "i32", "i64" (size_t is taken as 64-bit), "float", "double" or "void" """
    if "*" in text or "[" in text:
        return "pointer"
    words = [w for w in text.split() if w != "const"]
    base = words[0] if len(words) == 1 else " ".join(words[:-1])  # a return type stands alone; a parameter carries its name
    return {"void": "void", "int": "i32", "unsigned": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64",
            "size_t": "i64", "float": "float", "double": "double"}[base]


def c_kind_of_ctype(t):
    """the same kinds for a ctypes type of an argtypes list or a restype"""
    if t is None:
        return "void"
    code = getattr(t, "_type_", None)
    if not isinstance(code, str):
        assert issubclass(t, C._Pointer), t
        return "pointer"
    return {"f": "float", "d": "double", "P": "pointer", "z": "pointer"}.get(code) or {4: "i32", 8: "i64"}[C.sizeof(t)]


def c_zero_args(argtypes):
    """zero for every numeric kind and None for every pointer: the arguments of the null-handle census"""
    return [None if c_kind_of_ctype(a) == "pointer" else 0 for a in argtypes]


def run_ldpc_planner(exe, rows, group_size=32):
    """rows: (table, {override: value}). One dict per row: {"error": text}, or name / dmax / words_per_check / pr_shared_sv / lds_bytes /
    gsync_on, `check` (first broken format invariant, "" = none) and recs / wrecs, the truncated sha256 of the record words."""
    text = "".join("%s %d %s\n" % (t, group_size, " ".join("%s=%s" % kv for kv in sorted(env.items()))) for t, env in rows)
    r = subprocess.run([exe], input=text.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr
    out, pos, plans = r.stdout, 0, []
    while pos < len(out):
        end = out.index(b"\n", pos)
        kind, line = out[pos:pos + 1], out[pos + 2:end].decode()
        pos = end + 1
        if kind == b"E":
            plans.append({"error": line})
            continue
        f = line.split("|")
        n_recs, n_wrecs = int(f[6]), int(f[7])
        recs, wrecs = out[pos:pos + 4 * n_recs], out[pos + 4 * n_recs:pos + 4 * (n_recs + n_wrecs)]
        pos += 4 * (n_recs + n_wrecs)
        plans.append({"name": f[0], "dmax": int(f[1]), "words_per_check": int(f[2]), "pr_shared_sv": int(f[3]), "lds_bytes": int(f[4]), "gsync_on": int(f[5]),
                      "check": f[8] if len(f) > 8 else "", "recs": hashlib.sha256(recs).hexdigest()[:12], "wrecs": hashlib.sha256(wrecs).hexdigest()[:12]})
    assert len(plans) == len(rows)
    return plans


# ------------------------------------------------------------------ device buffers of the stage tests (torch is imported where it is used)
SENTINEL = 0xC3A55A3C  # a bit pattern no output of the stage tests holds
PAD = 64               # sentinel elements behind the last output of run_strided


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sentinel(n_words):
    """n_words 32-bit words of SENTINEL on the device, as int32 (torch has no uint32 arithmetic worth the name); a complex element is two"""
    import torch
    return torch.full((n_words,), np.uint32(SENTINEL).astype(np.int32).item(), dtype=torch.int32, device="cuda")


def refused(code, text, entry, *args):
    """the C entry answers `code` and leaves exactly `text` behind"""
    from dvbs2rx_amd import capi
    assert entry(*args) == code, (entry.__name__, capi.lib.dvbs2_last_error())
    assert capi.lib.dvbs2_last_error() == text.encode(), capi.lib.dvbs2_last_error()


def same_bits(got, want_bits, what):
    """got: uint32 (n, 2) complex samples read back from the device; want_bits: the model's samples as uint32 (the model's bits())"""
    w = want_bits.reshape(-1, 2)
    assert got.shape[0] == w.shape[0], (what, got.shape[0], w.shape[0])
    if not np.array_equal(got, w):
        bad = np.nonzero((got != w).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {w.shape[0]} samples differ, the first at {bad[0]}: {got[bad[0]]} != {w[bad[0]]}")


def run_strided(call, xs, counts, in_stride, out_stride, in_shift=0, out_shift=0):
    """One device call over the input streams xs (complex64 vectors of one length) into len(counts) outputs. Input i lies at in_shift +
    i * in_stride complex elements of a 16-byte-aligned buffer; output s is counts[s] elements at out_shift + s * out_stride of a
    16-byte-aligned sentinel buffer. call(in_ptr, out_ptr) makes the call. Returns (one uint32 (counts[s], 2) array per output, what call
    returned) after checking that everything else in the output buffer -- the shift in front, what lies between and behind the outputs and
    PAD elements behind the last stride -- is still the sentinel, and that the input is unchanged."""
    import torch
    n = xs[0].size
    host_in = np.full(in_shift + len(xs) * in_stride + 2, np.complex64(complex(9.5, -9.5)), np.complex64)
    for i, x in enumerate(xs):
        assert x.size == n
        host_in[in_shift + i * in_stride:in_shift + i * in_stride + n] = x
    d_in = torch.from_numpy(host_in.view(np.float32)).cuda()
    n_buf = out_shift + max(len(counts), 1) * out_stride + PAD
    d_out = sentinel(2 * n_buf)
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    ret = call(d_in.data_ptr() + 8 * in_shift, d_out.data_ptr() + 8 * out_shift)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), host_in.view(np.uint32)), "the input was written"
    touched = np.zeros(n_buf, bool)
    outs = []
    for s, k in enumerate(counts):
        a = out_shift + s * out_stride
        touched[a:a + k] = True
        outs.append(got[a:a + k])
    assert (got[~touched] == SENTINEL).all(), "a write outside the outputs"
    return outs, ret


# ------------------------------------------------------------------ input generators
def llr_noise(n_frames, N, seed, sigma=8.0):
    """Never-converging input of SURVEY 8(d): i.i.d. clamp(round(N(0, sigma^2)))."""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, sigma, (n_frames, N))), -128, 127).astype(np.int8)


def ldpc_encode(table, info_bits):
    """info_bits: (n_frames, K) uint8 in {0,1} -> codeword bits (n_frames, N)."""
    N, K, _, _ = ldpc_info(table)
    cw = np.zeros((info_bits.shape[0], N), np.uint8)
    for f in range(info_bits.shape[0]):
        assert oracle().oracle_ldpc_encode(table.encode(), ptr(np.ascontiguousarray(info_bits[f])), ptr(cw[f])) == 0
    return cw


def llr_codeword_awgn(table, n_frames, seed, amp=6.0, sigma=4.0, info=None):
    """Valid codewords through a BPSK-like AWGN channel quantised to int8 (bit 0 -> +amp)."""
    N, K, _, _ = ldpc_info(table)
    rng = np.random.default_rng(seed)
    if info is None:
        info = rng.integers(0, 2, (n_frames, K), dtype=np.uint8)
    cw = ldpc_encode(table, info)
    y = amp * (1.0 - 2.0 * cw) + sigma * rng.normal(0.0, 1.0, cw.shape)
    return np.clip(np.rint(y), -128, 127).astype(np.int8), cw


def make_input(table, kind, n_frames, seed=0, amp=6.0, sigma=4.0):
    """Deterministic LDPC test inputs by name (used by the golden fixtures)."""
    N = ldpc_info(table)[0]
    if kind == "noise":
        return llr_noise(n_frames, N, seed)
    if kind == "awgn":
        return llr_codeword_awgn(table, n_frames, seed, amp=amp, sigma=sigma)[0]
    if kind == "sat":
        rng = np.random.default_rng(seed)
        return rng.choice(np.array([-128, -127, 127, 126, 0], np.int8), (n_frames, N))
    if kind == "zero":
        return np.zeros((n_frames, N), np.int8)
    if kind == "clean":  # valid codewords with strong LLRs: the first syndrome test passes, zero updates
        return llr_codeword_awgn(table, n_frames, seed, amp=20, sigma=0.0)[0]
    raise ValueError(kind)


# ------------------------------------------------------------------ BCH helpers (oracle)
class OracleBch:
    def __init__(self, m, prim_poly, t, n=0):
        self.o = oracle()
        self.h = self.o.oracle_bch_new(m, prim_poly, t, n)
        self.n, self.k, self.t, self.m = self.o.oracle_bch_n(self.h), self.o.oracle_bch_k(self.h), t, m

    def __del__(self):
        try:
            self.o.oracle_bch_free(self.h)
        except Exception:
            pass

    def genpoly_int(self):
        deg = self.o.oracle_bch_gdeg(self.h)
        g = np.zeros(deg + 1, np.uint8)
        self.o.oracle_bch_genpoly(self.h, ptr(g))
        return sum(int(b) << i for i, b in enumerate(g))

    def alpha(self, i):
        return self.o.oracle_bch_alpha(self.h, i)

    def minpoly(self, e):
        return self.o.oracle_bch_minpoly(self.h, e)

    def encode_bits(self, msg_bits):
        cw = np.zeros(self.n, np.uint8)
        self.o.oracle_bch_encode_bits(self.h, ptr(np.ascontiguousarray(msg_bits, np.uint8)), ptr(cw))
        return cw

    def syndrome_bits(self, cw_bits):
        S = np.zeros(2 * self.t, np.uint32)
        n = self.o.oracle_bch_syndrome_bits(self.h, ptr(np.ascontiguousarray(cw_bits, np.uint8)), ptr(S))
        return S[:n]

    def err_loc(self, S):
        sigma = np.zeros(64, np.uint32)
        deg = self.o.oracle_bch_err_loc_poly(self.h, ptr(np.ascontiguousarray(S, np.uint32)), ptr(sigma))
        nums = np.zeros(32, np.uint32)
        cnt = self.o.oracle_bch_err_loc_numbers(self.h, ptr(sigma), deg, ptr(nums))
        return sigma[:deg + 1], nums[:max(cnt, 0)], cnt

    def encode_bytes(self, msg):
        msg = np.ascontiguousarray(msg, np.uint8)
        cw = np.zeros((msg.shape[0], self.n // 8), np.uint8)
        for f in range(msg.shape[0]):
            self.o.oracle_bch_encode_bytes(self.h, ptr(msg[f]), ptr(cw[f]))
        return cw

    def decode_bytes(self, cw):
        cw = np.ascontiguousarray(cw, np.uint8)
        msg = np.zeros((cw.shape[0], self.k // 8), np.uint8)
        ret = np.zeros(cw.shape[0], np.int32)
        for f in range(cw.shape[0]):
            ret[f] = self.o.oracle_bch_decode_bytes(self.h, ptr(cw[f]), ptr(msg[f]))
        return msg, ret

    # the interface of RefBch, so that either one serves as the checker (bch_checker)
    def encode(self, msg):
        return self.encode_bytes(np.reshape(msg, (-1, self.k // 8)))

    def decode(self, cw):
        msg, ret = self.decode_bytes(np.reshape(cw, (-1, self.n // 8)))
        return msg, ret.tolist()

    def close(self):
        pass


def bch_golden_input(codec, n, k, case):
    """Received word of one tests/golden/bch_golden.json case. codec: anything with encode_bytes()/encode() (the
    systematic encoder is pinned by the reference's own KATs and by the committed sha_in)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bch_craft
    if "exps" in case:
        return bch_craft.word_from_exponents(n, case["exps"])
    if case.get("garbage"):
        return np.random.default_rng(case["seed"]).integers(0, 256, n // 8, dtype=np.uint8)
    msg = np.random.default_rng(case["seed"]).integers(0, 256, (1, k // 8), dtype=np.uint8)
    cw = codec.encode(msg)[0] if hasattr(codec, "encode") else codec.encode_bytes(msg)[0]
    return flip_bits(cw, case["flips"])


def chain_expect(table, bch_n, bch_t, framesize, llr, trials):
    """What ldpc_decoder_bb (OM_MESSAGE) -> bch_decoder_bb give for a WHOLE batch of int8 LLR frames, G = 32: the genuine
    AVX2 LDPC reference on all cores (the restatement without oracle/_ref), then the BCH codec frame by frame (the genuine
    bch.cc when oracle/_ref holds it, else the restatement). Returns (messages, corrections per frame, LDPC return values,
    who)."""
    if ref_ldpc() is not None:
        dec_llr, wret = ref_ldpc_decode_parallel(table, llr, 0, trials); who = "reference AVX2 LDPC"
    else:
        dec_llr, wret = oracle_ldpc_decode(table, llr, 32, trials); who = "oracle LDPC"
    cw = pack_bits(dec_llr, bch_n)
    m, prim = BCH_FIELDS[framesize]
    if ref_bch() is not None:
        rb = RefBch(prim, bch_t, bch_n)
        msg, corr = rb.decode(cw)
        rb.close()
        return msg, np.asarray(corr, np.int32), wret, who + " + reference BCH"
    msg, corr = OracleBch(m, prim, bch_t, bch_n).decode_bytes(cw)
    return msg, corr, wret, who + " + BCH oracle"


BCH_FIELDS = {1: (16, 0b10000000000101101), 0: (14, 0b100000000101011), 2: (15, 0b1000000000101101)}  # by framesize id


# ------------------------------------------------------------------ BCH: every outer code, planted received words
def bch_codes():
    """One row of tests/golden/fec_params.json per distinct (framesize, bch_n, bch_k, bch_t) that the byte API accepts (n and k
    multiples of 8, lib/bch.cc:19-24): the normal and short codes of DVB-S2, S2X and T2. Medium frames are refused like the
    reference. The first row of each code is kept; its standard, rate and LDPC table feed the chain tests."""
    import json
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "fec_params.json")))["rows"]
    seen, out = set(), []
    for r in rows:
        key = (r["framesize_id"], r["bch_n"], r["bch_k"], r["bch_t"])
        if key in seen or r["bch_n"] % 8 or r["bch_k"] % 8:
            continue
        seen.add(key)
        out.append(r)
    return out


def bch_checker(m, prim_poly, t, n):
    """The expected results of a BCH code: the genuine reference codec (RefBch) where oracle/_ref holds it, else the plain-C
    restatement (OracleBch, pinned to the genuine codec by tests/golden/bch_golden.json). Returns (codec, name); both codecs
    offer encode(msg) and decode(cw) -> (msg, list of return values)."""
    if ref_bch() is not None:
        return RefBch(prim_poly, t, n), "RefBch"
    return OracleBch(m, prim_poly, t, n), "OracleBch"


_craft_cache = {}


def bch_crafted(m, prim_poly, n, t):
    """The two words of tools/bch_craft.py on which the reference throws for this code (decode() -2), as packed rows: "quadratic"
    (a degree-2 locator without roots) and "beyond_n" (one error location >= n). Deterministic, cached."""
    key = (m, prim_poly, n, t)
    if key not in _craft_cache:
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bch_craft
        if (m, prim_poly) not in _craft_cache:
            _craft_cache[(m, prim_poly)] = bch_craft.GF(m, prim_poly)
        gf = _craft_cache[(m, prim_poly)]
        rng = np.random.default_rng(7919 * n + t)
        _craft_cache[key] = (bch_craft.word_from_exponents(n, bch_craft.craft_quadratic(gf, n, t, rng)),
                             bch_craft.word_from_exponents(n, bch_craft.craft_beyond_n(gf, n, t, rng)))
    return _craft_cache[key]


class BchPlanted:
    """Received words of one BCH code: rx (W, n/8); msg (W, k/8), the message each word was made from (zero for garbage and
    crafted words); planted, the error count of each word, None where the word is not a codeword plus <= t errors; names."""

    def __init__(self, rx, msg, planted, names):
        self.rx, self.msg, self.planted, self.names = rx, msg, planted, names

    def correctable(self):
        return [i for i, c in enumerate(self.planted) if c is not None]


def bch_planted(codec, m, prim_poly, t, seed=None):
    """THE planted words of a BCH code (codec: the checker, for encode(), n and k), 33 of them, deterministic per code:
      0, 1, 2, 3, 4, 5, t-1, t, t+1, t+2, 2t and 40 errors at random positions;
      single errors at stream positions 0, n-1, k-1, k and on byte edges (7, 8, k-8, k+7), pairs at (0, n-1), (k-1, k) and on
      byte edges;
      both sides of the first column of each of the last two 128-column steps of the syndrome product, and the last column
      before its padding (n-1) together with the first column of the last step;
      three parity-only errors, a burst of t;
      one garbage word and the two crafted words on which the reference throws (the last two)."""
    n, k = codec.n, codec.k
    rng = np.random.default_rng(13 * n + t if seed is None else seed)
    steps = (n + 127) // 128
    pats = [(f"random {c}", rng.choice(n, c, replace=False)) for c in (0, 1, 2, 3, 4, 5, t - 1, t, t + 1, t + 2, 2 * t, 40)]
    pats += [(f"single at {p}", [p]) for p in (0, n - 1, k - 1, k, 7, 8, k - 8, k + 7)]
    pats += [(f"pair at {a}, {b}", [a, b]) for a, b in ((0, n - 1), (k - 1, k), (7, 8), (k - 9, k - 8), (n - 9, n - 8))]
    pats += [(f"step edge {b}", [b - 1, b]) for b in ((steps - 2) * 128, (steps - 1) * 128) if b >= 1]
    pats.append(("last column + last step", [(steps - 1) * 128, n - 1]))
    pats.append(("parity only", k + rng.choice(n - k, 3, replace=False)))
    b0 = int(rng.integers(0, n - t))
    pats.append(("burst of t", list(range(b0, b0 + t))))
    msg = rng.integers(0, 256, (len(pats) + 3, k // 8), dtype=np.uint8)
    cw = codec.encode(msg[:len(pats)])
    rx, planted, names = [], [], []
    for i, (name, pos) in enumerate(pats):
        pos = sorted({int(p) for p in pos})
        assert all(0 <= p < n for p in pos), (name, pos)
        rx.append(flip_bits(cw[i], pos))
        planted.append(len(pos) if len(pos) <= t else None)
        names.append(name)
    rx.append(rng.integers(0, 256, n // 8, dtype=np.uint8))
    rx += list(bch_crafted(m, prim_poly, n, t))
    names += ["garbage", "throw quadratic", "throw beyond n"]
    planted += [None] * 3
    msg[len(pats):] = 0
    return BchPlanted(np.stack(rx), msg, planted, names)


def bch_assert_truth(pl, out, ret, what=""):
    """Every word of <= t planted errors decodes to the sent message with the planted count (independent of any checker)."""
    ok = pl.correctable()
    bad = [(pl.names[i], int(ret[i]), pl.planted[i]) for i in ok if int(ret[i]) != pl.planted[i]]
    assert not bad, (what, bad)
    bad = [pl.names[i] for i in ok if not np.array_equal(out[i], pl.msg[i])]
    assert not bad, (what, bad)


def flip_bits(cw_bytes, positions):
    """Flip stream bit positions (0 = first transmitted bit) in a packed byte row (copy)."""
    out = cw_bytes.copy()
    for p in positions:
        out[p // 8] ^= np.uint8(1 << (7 - p % 8))
    return out


# ------------------------------------------------------------------ demapper helpers (oracle)
def oracle_demap(syms, n0, constellation, order=0):
    syms = np.ascontiguousarray(syms, np.complex64)
    nf, ns = syms.shape
    n0 = np.broadcast_to(np.asarray(n0, np.float32), (nf,))
    nmod = 2 if constellation == 4 else 3
    out = np.zeros((nf, ns * nmod), np.int8)
    for f in range(nf):
        if constellation == 4:
            oracle().oracle_demap_qpsk(ptr(syms[f]), ns, float(n0[f]), ptr(out[f]))
        else:
            oracle().oracle_demap_8psk(ptr(syms[f]), ns, float(n0[f]), order, ptr(out[f]))
    return out


M8PSK = np.array([np.sqrt(.5) * (1 + 1j), 1, -1, np.sqrt(.5) * (-1 - 1j), 1j, np.sqrt(.5) * (1 - 1j),
                  np.sqrt(.5) * (-1 + 1j), -1j], np.complex64)


def map_8psk(bits3):
    """bits3: (..., 3) bits (b0 b1 b2 of lib/psk.hh:152-157 in +-1 -> index form) -> constellation point."""
    b = 1 - 2 * bits3.astype(np.int32)  # bit 0 -> +1, bit 1 -> -1 (positive LLR = bit 0)
    idx = (((b[..., 0] + 1) << 1) ^ 0x4) | ((b[..., 1] + 1) ^ 0x2) | (((b[..., 2] + 1) >> 1) ^ 0x1)
    return M8PSK[idx]


# ------------------------------------------------------------------ demapper: float64 reference of the formulas
# The restatement above (oracle/demap_oracle.c) and the kernels (demap_math.hpp) evaluate the reference's formulas in float32.
# What follows evaluates the same formulas in float64 -- the mathematics, not a second float32 restatement -- plus a float32
# emulation in numpy (IEEE single operations, no FMA, the operation order of demap_math.hpp) used to construct exact ties.
U32 = 2.0 ** -24  # unit roundoff of float32 (round to nearest)
RS2_F32 = float(np.float32(0.70710678118654752440))  # the reference points are float constants (lib/psk.hh, lib/qpsk.h)
COS_PI_8, SIN_PI_8 = np.cos(np.pi / 8), np.sin(np.pi / 8)
SNR_FLOOR = float(np.float32(1e-12))  # noise power floor, lib/qpsk.h:61-62, lib/xfecframe_demapper_cb_impl.cc:141-143

# 8PSK column order by RATE NAME (reference lib/xfecframe_demapper_cb_impl.cc:50-69): 0 = "012", 1 = "210", 2 = "102"
COLUMN_ORDER_210 = ("C3_5",)
COLUMN_ORDER_102 = ("C25_36", "C13_18", "C7_15", "C8_15", "C26_45")


def column_order(rate_name):
    return 1 if rate_name in COLUMN_ORDER_210 else 2 if rate_name in COLUMN_ORDER_102 else 0


def column_bases(rows, order):
    """(ra0, ra1, ra2): where bits b0, b1, b2 of symbol s land in the de-interleaved frame (ra_k + s)."""
    return {0: (0, rows, 2 * rows), 1: (2 * rows, rows, 0), 2: (rows, 0, 2 * rows)}[order]


def _n0_f64(n0, nf):
    # N0 is a float in the block (d_N0); the formulas see that float value
    return np.broadcast_to(np.asarray(n0, np.float32), (nf,)).astype(np.float64)[:, None]


def _rotate_f64(syms):
    re, im = syms.real.astype(np.float64), syms.imag.astype(np.float64)
    return re * COS_PI_8 + im * SIN_PI_8, -re * SIN_PI_8 + im * COS_PI_8  # x * exp(-j pi/8)


def demap_f64(syms, n0, constellation, order=0):
    """UNQUANTISED LLRs in float64, (n_frames, n_llr), in the block's output order. constellation: 4 (QPSK) or 8 (8PSK).
    QPSK  x * 2 sqrt(2) / N0 on re, im of each symbol (reference lib/qpsk.h:208-214).
    8PSK  c = x exp(-j pi/8); b1 = Re c * D, b2 = Im c * D, b0 = (|Re c| - |Im c|) / sqrt(2) * D, D = 2 sin(pi/8) * 4 / N0
          (lib/psk.hh:113-150, precision 4 / N0 at lib/xfecframe_demapper_cb_impl.cc:148); bit k of symbol s at ra_k + s
          (:50-69, 162-176)."""
    syms = np.asarray(syms, np.complex64)
    nf, ns = syms.shape
    n0 = _n0_f64(n0, nf)
    if constellation == 4:
        out = np.empty((nf, 2 * ns))
        S = 2.0 * np.sqrt(2.0) / n0
        out[:, 0::2], out[:, 1::2] = syms.real * S, syms.imag * S
        return out
    D = 2.0 * SIN_PI_8 * 4.0 / n0
    cr, ci = _rotate_f64(syms)
    ra = column_bases(ns, order)
    out = np.empty((nf, 3 * ns))
    for a, v in zip(ra, ((np.abs(cr) - np.abs(ci)) / np.sqrt(2.0) * D, cr * D, ci * D)):
        out[:, a:a + ns] = v
    return out


def quantise_f64(v):
    """clamp(rint(v), -128, 127) with ties to even (rintf / nearbyintf / VOLK's convert)."""
    return np.clip(np.rint(v), -128, 127).astype(np.int8)


def near_tie_mask(syms, n0, constellation, order=0):
    """Positions where a float32 evaluation of the formulas may quantise differently from quantise_f64(demap_f64(...)).

    The bound is on the INPUT magnitudes A = |re| + |im| of the symbol (u = 2^-24): 8PSK cancels in re rr - im ri and in
    |cr| - |ci|, so an error relative to the output is not a bound.
      QPSK  scalar = fl(2 sqrt(2) / N0) = S (1 + d1); v = fl(x scalar): |v - x S| <= (2u + u^2) |x| S.      k = 3
      8PSK  rr, ri are float roundings of cos, sin (u each); the two products (u each) and the sum / difference (u):
            |cr32 - cr| <= 3.01 u A, same for ci. dp = fl(fl(2 sin_pi_8) fl(4 / N0)) = D (1 + e), |e| <= 3.01 u.
            b1, b2 = fl(c dp):               <= 3.01 u A D + 4.01 u |c| D                      <= 7.02 u A D
            w = fl(|cr32| - |ci32|):         |w - (|cr| - |ci|)| <= 6.02 u A + u A            =  7.02 u A
            z = fl(fl(1/sqrt 2) w):          <= (7.02 + 2.01) u A / sqrt 2                    <= 6.39 u A
            b0 = fl(z dp):                   <= 6.39 u A D + 4.01 u (A / sqrt 2) D            <= 9.23 u A D    k = 10
    plus an absolute term for products that land in the subnormal range (each rounds by <= 2^-150, scaled by D).
    Quantisation is clamp(rint(v)): it is discontinuous only at the half-integers -127.5 .. 126.5 (at -128.5 and 127.5 rint and
    clamp agree); the mask takes every half-integer from -128.5 to 127.5, so it also covers the saturation points. Non-finite
    values are exact (+-inf saturates either way) and never near."""
    syms = np.asarray(syms, np.complex64)
    nf, ns = syms.shape
    v = demap_f64(syms, n0, constellation, order)
    n0 = _n0_f64(n0, nf)
    if constellation == 4:
        S = 2.0 * np.sqrt(2.0) / n0
        a = np.empty_like(v)
        a[:, 0::2], a[:, 1::2] = np.abs(syms.real), np.abs(syms.imag)
        margin = 3 * U32 * a * S + 2.0 ** -149
    else:
        D = 2.0 * SIN_PI_8 * 4.0 / n0
        A = np.abs(syms.real).astype(np.float64) + np.abs(syms.imag)
        m = 10 * U32 * A * D + 2.0 ** -147 * D + 2.0 ** -149
        margin = np.concatenate([m, m, m], axis=1)  # the same bound in every column
    with np.errstate(invalid="ignore"):
        d = np.where(v < -128.5, -128.5 - v, np.where(v > 127.5, v - 127.5, np.abs(v - (np.floor(v) + 0.5))))
        return np.isfinite(v) & (d <= margin)


def check_demap_vs_f64(got, syms, n0, constellation, order=0, what=""):
    """Every LLR outside near_tie_mask equals quantise_f64(demap_f64(...)); near-tie ones are within +-1. Returns the near-tie count."""
    want = quantise_f64(demap_f64(syms, n0, constellation, order))
    near = near_tie_mask(syms, n0, constellation, order)
    diff = got.astype(np.int16) - want
    far_bad = np.nonzero((diff != 0) & ~near)
    assert far_bad[0].size == 0, f"{what}: {far_bad[0].size} LLRs differ away from a tie, first at {far_bad[0][0]}, {far_bad[1][0]}"
    assert np.abs(diff[near]).max(initial=0) <= 1, what
    return int(near.sum())

def demap_f32_pre(syms, n0, constellation):
    """The float32 values just before rint, emulated in numpy (IEEE single operations, no FMA, demap_math.hpp's order), for a
    single N0. QPSK: (..., 2 n) interleaved; 8PSK: (b0, b1, b2) per symbol, natural order."""
    syms = np.asarray(syms, np.complex64)
    f = np.float32
    n0 = f(n0)
    re, im = syms.real.astype(f), syms.imag.astype(f)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if constellation == 4:
            S = f(2.0 * 1.41421356237309504880 / np.float64(n0))
            out = np.empty(syms.shape[:-1] + (2 * syms.shape[-1],), f)
            out[..., 0::2], out[..., 1::2] = re * S, im * S
            return out
        rr, ri = f(np.cos(-np.pi / 8)), f(np.sin(-np.pi / 8))
        dp = f(f(2 * f(0.38268343236508977173)) * f(4.0 / np.float64(n0)))
        cr = re * rr - im * ri
        ci = re * ri + im * rr
        return f(0.70710678118654752440) * (np.abs(cr) - np.abs(ci)) * dp, cr * dp, ci * dp


def tie_symbols(n0, constellation, targets=None, reach=512):
    """Symbols whose float32 product lands EXACTLY on a tie t = k + 0.5 (default: every k in -129 .. 127), for one N0.
    QPSK: x on one axis. 8PSK: (x, 0) for b1 and, for positive b0, the b0 search; (0, x) for b2 and for negative b0 (b0 has
    the sign of |cos| - |sin| there). Each candidate x is searched over +-reach float32 steps around t / gain.
    Returns {t: complex64 symbol} for the ties found."""
    f = np.float32
    if targets is None:
        targets = np.arange(-129, 128) + 0.5
    n0 = f(n0)
    D = float(f(f(2 * f(0.38268343236508977173)) * f(4.0 / np.float64(n0))))
    S = float(f(2.0 * 1.41421356237309504880 / np.float64(n0)))
    if constellation == 4:
        combos = [(0, 1, S), (1, 1, S)]  # (axis, output index in the pair, gain)
    else:
        c, s = COS_PI_8, SIN_PI_8
        combos = [(0, 1, c * D), (0, 0, (c - s) / np.sqrt(2) * D), (1, 2, c * D), (1, 0, (s - c) / np.sqrt(2) * D)]
    steps = np.arange(-reach, reach + 1, dtype=np.int64)
    found = {}
    for t in targets:
        for axis, which, gain in combos:
            x0 = t / gain
            if not np.isfinite(x0) or abs(x0) >= 3e38 or x0 == 0:
                continue
            mag = (np.abs(np.float32(x0)).view(np.int32).astype(np.int64) + steps)
            mag = mag[(mag > 0) & (mag < 0x7f800000)].astype(np.int32).view(np.float32)
            x = np.sign(x0).astype(np.float32) * mag
            sy = (x + 0j).astype(np.complex64) if axis == 0 else (1j * x).astype(np.complex64)
            pre = demap_f32_pre(sy, n0, constellation)
            v = pre[1::2] if (constellation == 4 and axis == 1) else pre[0::2] if constellation == 4 else pre[which]
            hit = np.nonzero(v == np.float32(t))[0]
            if hit.size:
                found[float(t)] = sy[hit[0]]
                break
    return found


def edge_symbols(n0, constellation):
    """Symbols at the quantiser's edges for one N0: every exact tie found, far beyond saturation, +-0 in every combination,
    zero, the smallest subnormal, and (QPSK only: 8PSK turns inf into NaN through |cr| - |ci|) +-inf."""
    ties = list(tie_symbols(n0, constellation).values())
    big = [1e3, -1e3, 3e38, -3e38]
    z = [complex(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0)]
    tiny = [complex(1e-45, -1e-45), complex(-1e-45, 1e-45)]
    extra = [complex(b, 0) for b in big] + [complex(0, b) for b in big] + [complex(b, -b) for b in big[:2]] + z + tiny
    if constellation == 4:
        extra += [complex(np.inf, -np.inf), complex(-np.inf, np.inf), complex(np.inf, 0.0), complex(0.0, -np.inf)]
    out = np.array(ties + extra, np.complex64)
    # complex(a, b) drops the sign of a -0.0 real part in some paths: set the +-0 ones explicitly
    k0 = len(ties) + 10
    out.real[k0:k0 + 4] = np.array([0.0, 0.0, -0.0, -0.0], np.float32)
    out.imag[k0:k0 + 4] = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    return out


def snr_f64(syms, constellation, ref_llr=None, order=0):
    """Linear SNR per frame in float64: reference points by hard slice of the symbol (pre-decoder, lib/qpsk.h:171-181,
    lib/xfecframe_demapper_cb_impl.cc:132-141) or re-mapped from the signs of ref_llr (post-decoder, :268-307, lib/qpsk.h:266-281;
    LLR 0 counts as positive), then sum |s|^2 / sum |x - s|^2 with the noise floored at (float)1e-12. The points are the float
    constants of the reference's tables (M8PSK, RS2_F32), exactly as the block holds them."""
    syms = np.asarray(syms, np.complex64)
    nf, ns = syms.shape
    re, im = syms.real.astype(np.float64), syms.imag.astype(np.float64)
    if constellation == 4:
        if ref_llr is None:
            pr, pi = re >= 0, im >= 0
        else:
            ref_llr = np.asarray(ref_llr)
            pr, pi = ref_llr[:, 0::2] >= 0, ref_llr[:, 1::2] >= 0
        sr, si = np.where(pr, RS2_F32, -RS2_F32), np.where(pi, RS2_F32, -RS2_F32)
    else:
        if ref_llr is None:
            cr, ci = _rotate_f64(syms)
            b0, b1, b2 = np.where(np.abs(cr) < np.abs(ci), -1, 1), np.where(cr < 0, -1, 1), np.where(ci < 0, -1, 1)
        else:
            ra = column_bases(ns, order)
            b0, b1, b2 = (np.where(np.asarray(ref_llr)[:, a:a + ns] < 0, -1, 1) for a in ra)
        idx = (((b0 + 1) << 1) ^ 0x4) | ((b1 + 1) ^ 0x2) | (((b2 + 1) >> 1) ^ 0x1)
        pts = M8PSK.astype(np.complex128)[idx]
        sr, si = pts.real, pts.imag
    sp = (sr * sr + si * si).sum(axis=1)
    npow = ((re - sr) ** 2 + (im - si) ** 2).sum(axis=1)
    npow = np.where(npow > 0, npow, SNR_FLOOR)
    return sp / npow


def oracle_snr(syms, constellation, ref_llr=None, order=0):
    """oracle_demap_snr / oracle_demap_snr_refined per frame (float32, sequential accumulation)."""
    syms = np.ascontiguousarray(syms, np.complex64)
    nf, ns = syms.shape
    if ref_llr is None:
        return np.array([oracle().oracle_demap_snr(ptr(syms[f]), ns, constellation) for f in range(nf)], np.float64)
    ref_llr = np.ascontiguousarray(ref_llr, np.int8)
    return np.array([oracle().oracle_demap_snr_refined(ptr(syms[f]), ptr(ref_llr[f]), ns, constellation, order) for f in range(nf)],
                    np.float64)


def oracle_bb_descramble(msg):
    """msg: (n_frames, kbch_bytes) uint8 -> descrambled copy (lib/bbdescrambler_bb_impl.cc:67-82)."""
    msg = np.ascontiguousarray(msg, np.uint8)
    out = np.empty_like(msg)
    oracle().oracle_bb_descramble(ptr(msg), ptr(out), msg.shape[1], msg.shape[0])
    return out


def oracle_pl_payload(payload, n_slots, has_pilots, gold, plheader_phase, fine_foffset, coarse, pilot_phase):
    """payload: (n_frames, payload_len) complex64 -> (n_frames, 90 n_slots) complex64 (lib/plsync_cc_impl.cc:644-795)."""
    payload = np.ascontiguousarray(payload, np.complex64)
    nf = payload.shape[0]
    out = np.empty((nf, n_slots * 90), np.complex64)
    pp = np.ascontiguousarray(pilot_phase, np.float32)
    for f in range(nf):
        oracle().oracle_pl_payload(ptr(payload[f]), n_slots, int(has_pilots), gold, float(plheader_phase[f]), float(fine_foffset[f]),
                                   int(coarse[f]), ptr(np.ascontiguousarray(pp[f])), ptr(out[f]))
    return out


# ---- BBFRAME de-header (oracle/bbdeheader_oracle.c) -------------------------------------------------------------------
class _BbdhOracleState(C.Structure):
    _fields_ = [("kbch_bytes", C.c_int), ("max_dfl", C.c_int), ("synched", C.c_int), ("partial", C.c_int),
                ("partial_pkt", C.c_uint8 * 188), ("packets", C.c_uint64), ("errors", C.c_uint64), ("bbframes", C.c_uint64),
                ("dropped", C.c_uint64), ("gaps", C.c_uint64), ("overruns", C.c_uint64)]


class OracleBbDeheader:
    """The plain-C restatement of bbdeheader_bb (stateful like the block)."""

    def __init__(self, kbch_bits):
        self.s = _BbdhOracleState()
        oracle().oracle_bbdh_init(C.byref(self.s), kbch_bits)
        self.kbch_bytes = kbch_bits // 8
        self.max_out = ((kbch_bits - 80) // 8 + 187) // 188 * 188

    def work(self, bbframes):
        bb = np.ascontiguousarray(bbframes, np.uint8)
        nf = bb.size // self.kbch_bytes
        out = np.empty(max(nf, 1) * self.max_out, np.uint8)
        n = oracle().oracle_bbdh_work(C.byref(self.s), ptr(bb), nf, ptr(out))
        return out[:n].copy()

    def counters(self):
        s = self.s
        return dict(packets=s.packets, errors=s.errors, bbframes=s.bbframes, dropped=s.dropped, gaps=s.gaps, overruns=s.overruns,
                    synched=s.synched, partial_ts_bytes=s.partial)


def crc8_dvbs2(data):
    """CRC-8 of DVB-S2 (x^8 + x^7 + x^6 + x^4 + x^2 + 1, zero start, no reflection) of a bytes-like, bit-serial."""
    reg = 0
    for byte in bytes(data):
        for b in range(7, -1, -1):
            reg = (reg << 1) | ((byte >> b) & 1)
            if reg & 0x100:
                reg ^= 0x1D5
    for _ in range(8):  # append eight zero bits: remainder of data * x^8
        reg <<= 1
        if reg & 0x100:
            reg ^= 0x1D5
    return reg & 0xff


def ts_up_stream(n_ups, rng):
    """n_ups MPEG-TS user packets: sync byte, three zero bytes, 184 random bytes (as the reference's test builds them)."""
    ups = rng.integers(0, 256, (n_ups, 188), dtype=np.uint8)
    ups[:, 0] = 0x47
    ups[:, 1:4] = 0
    return ups.reshape(-1)


def ts_crc_encode(up_stream):
    """Mode adaptation: the sync byte of every user packet but the first is replaced by the CRC-8 of the preceding packet's
    187 bytes after its sync byte (EN 302 307-1 clause 5.1.4)."""
    s = np.array(up_stream, np.uint8).copy()
    n = s.size // 188
    for i in range(1, n):
        s[i * 188] = crc8_dvbs2(s[(i - 1) * 188 + 1:i * 188])
    return s


def bbheader(kbch_bits, syncd_bits, dfl_bits=None, upl_bits=188 * 8, matype1=0xF2, matype2=0, sync=0x47):
    """Ten BBHEADER bytes with a correct CRC-8: MATYPE (TS, SIS, CCM, roll-off 0.2), UPL, DFL, SYNC, SYNCD."""
    if dfl_bits is None:
        dfl_bits = kbch_bits - 80
    h = bytes([matype1, matype2, upl_bits >> 8, upl_bits & 0xff, dfl_bits >> 8, dfl_bits & 0xff, sync, syncd_bits >> 8, syncd_bits & 0xff])
    return np.frombuffer(h + bytes([crc8_dvbs2(h)]), np.uint8)


def bbframe_stream(kbch_bits, n_frames, up_stream, syncd_bits=0):
    """n_frames BBFRAMEs whose DATAFIELDs carry the CRC-encoded user packet stream back to back (maximum DFL); SYNCD follows
    from where the first packet of each DATAFIELD starts."""
    dfl_bytes = (kbch_bits - 80) // 8
    enc = ts_crc_encode(up_stream)
    assert enc.size >= n_frames * dfl_bytes
    frames = np.zeros((n_frames, kbch_bits // 8), np.uint8)
    off = 0
    for i in range(n_frames):
        frames[i, :10] = bbheader(kbch_bits, syncd_bits)
        frames[i, 10:] = enc[off:off + dfl_bytes]
        partial = (off + dfl_bytes) % 188
        syncd_bits = ((188 - partial) % 188) * 8  # (a packet that starts with the DATAFIELD: SYNCD = 0, EN 302 307-1 clause 5.1.6)
        off += dfl_bytes
    return frames


# ------------------------------------------------------------------ a busy non-blocking stream (tests/test_stream_order_gpu.py)
# A hold is a BOUNDED spin enqueued on a stream: what is enqueued behind it stays pending while the host goes on. There is no gate that
# waits for the host, on purpose: a test that dies between enqueue and release must not leave a wave spinning on the card.
HOLD_MIN_MS, HOLD_MAX_MS, HOLD_FACTOR = 20.0, 250.0, 20.0
_sleep_cal = {}


def side_stream():
    """a stream the null stream does not order itself against (torch's pool streams are created with hipStreamNonBlocking)"""
    import torch
    return torch.cuda.Stream()


def null_stream():
    import torch
    return torch.cuda.default_stream()


def sleep_calibration():
    """dict(cycles_per_ms, probe_cycles, probe_ms): torch.cuda._sleep's cycles per millisecond, measured once per session with two events
    around one _sleep on an idle stream (a short one first, so that no code object loads between the events)."""
    import torch
    if not _sleep_cal:
        s = side_stream()
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
            s.synchronize()
            cycles, ms = 1_000_000, 0.0
            for _ in range(4):  # lengthen the probe until it lasts 20 ms: the events' own resolution is then below a percent
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                torch.cuda._sleep(cycles)
                b.record(s)
                s.synchronize()
                ms = a.elapsed_time(b)
                if ms >= 20.0:
                    break
                cycles = int(cycles * max(2.0, 40.0 / max(ms, 1e-3)))
        assert ms > 0.0, "torch.cuda._sleep takes no time on this device"
        _sleep_cal.update(cycles_per_ms=cycles / ms, probe_cycles=cycles, probe_ms=ms)
        print(f"sleep calibration: {cycles} cycles took {ms:.3f} ms: {cycles / ms:.0f} cycles per ms")
    return _sleep_cal


def hold(stream, ms):
    """keeps `stream` busy for about `ms` milliseconds from the moment the device gets to it; returns at once"""
    import torch
    assert 0.0 < ms <= HOLD_MAX_MS, f"a hold of {ms} ms: cut the sequence, not the margin"
    cycles = int(ms * sleep_calibration()["cycles_per_ms"])
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def hold_for(host_ms):
    """the hold behind which a sequence is enqueued whose host side took host_ms on an idle stream: 20 times that for the jitter of a
    machine others are using, never below 20 ms"""
    return max(HOLD_MIN_MS, HOLD_FACTOR * host_ms)


def pending(stream):
    return not stream.query()


def hip_runtime():
    """ctypes handle of the HIP runtime this process already runs on (the one torch brought, which the library bound to)"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, f"expected one HIP runtime in the process, found {sorted(paths)}"
    rt = C.CDLL(paths.pop())
    rt.hipMemset.restype = C.c_int
    rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    rt.hipMemcpyAsync.restype = C.c_int
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rt.hipStreamSynchronize.restype = C.c_int
    rt.hipStreamSynchronize.argtypes = [C.c_void_p]
    return rt
