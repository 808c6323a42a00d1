#!/usr/bin/env python3
"""tools/node_census.py -- STATIC census of ONE regular-layer packed check node (check_node_v2), per degree, from the device code of a
sweep-kernel build (`llvm-objdump -d` of gr-dvbs2rx_amd/build/ldpc_inst_<DMAX>.o), by the issue-rate classes of tools/valu_census.py.

  python tools/node_census.py                       # degree class 8, <8, packed, solo> (table B4's build), all degrees it instantiates
  python tools/node_census.py --obj OTHER.o --dmax 16 --kernel "ldpc_layered_kernel<16, packed, solo>"

A node is found by its issue-priority marks (s_setprio 0 -> 1 -> 3, check_node_v2): the straight-line span between them that holds
packed instructions, DEG LLR byte reads and no barrier or branch; its "tail" is what follows the s_setprio 3 up to the next branch
(message packing). The degree is the number of ds_read_u8. "loop" is the rest of that layer's straight line path: the scalar and vector
instructions between the tail and the next node of the same layer (the switch, message stores, record prefetch) are NOT in it -- they
are shared by all degrees and counted in the whole-kernel census (profiles/valu_mix.json).
Cycles are per wave at the saturated rates (cycles per wave-instruction per SIMD); x 3 waves per SIMD = one SIMD's issue time per layer.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from valu_census import B, RATES, classify, short  # noqa: E402


def disassemble(obj):
    with tempfile.TemporaryDirectory() as td:
        fb, elf = os.path.join(td, "k.fatbin"), os.path.join(td, "k.elf")
        subprocess.check_call([B + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
        subprocess.check_call([B + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fb, "--output=" + elf])
        return subprocess.run([B + "llvm-objdump", "-d", elf], capture_output=True, text=True, check=True).stdout


def kernel_ops(dis, want):
    ops, name = [], None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = short(m.group(1))
            continue
        if name != want:
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$", line)
        if m:
            ops.append((m.group(1), m.group(2)))
    return ops


def tally(seg):
    c = collections.Counter()
    for op, _ in seg:
        if op.startswith("v_"):
            k = classify(op)
            c["full" if k == "unknown" else k] += 1
            if op.startswith("v_pk_"):
                c["pk"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("s_nop"):
            c["s_nop"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
    c["valu"] = c["full"] + c["half"] + c["quarter"]
    c["cycles"] = c["full"] * RATES["full"] + c["half"] * RATES["half"] + c["quarter"] * RATES["quarter"]
    return c


def nodes(ops):
    out = {}
    for i, (op, arg) in enumerate(ops):
        if op != "s_setprio" or not arg.startswith("0"):
            continue
        p1 = p3 = None
        for j in range(i + 1, min(len(ops), i + 1000)):
            o, a = ops[j]
            if o == "s_setprio":
                if a.startswith("1") and p1 is None:
                    p1 = j
                elif a.startswith("3"):
                    p3 = j
                    break
                else:
                    break
            if o in ("s_barrier",) or "branch" in o:
                break
        if p1 is None or p3 is None:
            continue
        body = ops[i:p3 + 1]
        if not any(o.startswith("v_pk_") for o, _ in body):
            continue
        deg = sum(1 for o, _ in body if o == "ds_read_u8")
        tail = []
        for o, a in ops[p3 + 1:]:
            if "branch" in o or o == "s_setprio":
                break
            tail.append((o, a))
        if deg and deg not in out:
            out[deg] = (tally(body), tally(tail))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", default=os.path.join(ROOT, "gr-dvbs2rx_amd", "build", "ldpc_inst_8.o"))
    ap.add_argument("--kernel", default="ldpc_layered_kernel<8, packed, solo>")
    ap.add_argument("--deg", type=int, default=0, help="only this degree")
    a = ap.parse_args()
    found = nodes(kernel_ops(disassemble(a.obj), a.kernel))
    if not found:
        sys.exit(f"no packed regular node found in {a.kernel} of {a.obj}")
    print(f"{a.kernel}  ({os.path.relpath(a.obj, ROOT)}; rates {RATES} cycles per wave-instruction per SIMD)")
    print(f"{'deg':>3} {'part':5} {'valu':>5} {'full':>5} {'half':>5} {'quart':>5} {'(pk)':>5} {'lds':>4} {'salu':>4} {'nop':>4} {'cycles':>7} {'x3 waves':>8}")
    for deg in sorted(found):
        if a.deg and deg != a.deg:
            continue
        body, tail = found[deg]
        tot = body + tail
        tot["cycles"] = body["cycles"] + tail["cycles"]
        for part, c in (("node", body), ("tail", tail), ("total", tot)):
            print(f"{deg:3d} {part:5} {c['valu']:5d} {c['full']:5d} {c['half']:5d} {c['quarter']:5d} {c['pk']:5d} {c['lds']:4d} {c['salu']:4d} "
                  f"{c['s_nop']:4d} {c['cycles']:7.1f} {3 * c['cycles']:8.0f}")


if __name__ == "__main__":
    main()
