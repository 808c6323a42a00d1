#!/usr/bin/env python3
"""tools/trip_census.py -- STATIC census of what a wave issues per trip in three places of a packed sweep-kernel build, from the device
code of gr-dvbs2rx_amd/build/ldpc_inst_<DMAX>.o, by the issue-rate classes of tools/valu_census.py (sibling of tools/node_census.py,
which counts the regular node alone).

  python tools/trip_census.py                       # <8, packed, solo> (table B4's build), degree 7
  python tools/trip_census.py --obj OTHER.o --kernel "ldpc_layered_kernel<8, packed>" --deg 7

 (a) one REGULAR layer trip of the given degree: the cycle of basic blocks through the packed node (check_node_v2, found by its issue
     priority marks as in node_census.py) that a layer of that degree runs in every sweep but a frame's first -- the cheapest cycle of the
     control-flow graph through the node's block (the first body of the degree in address order: the run loop's where the build has
     one) that loads messages, stores messages (a frame's first sweep loads none) and meets no barrier; the blocks it takes and the
     form of every body found are printed, so the choice can be checked against the disassembly. Split into "node"
     (s_setprio 0 .. the end of the node's block: the node and its message packing, what node_census.py calls total) and "else"
     (everything outside: the layer head, the switch, message load / store, the copies at the loop's back edge).
 (a') where the build has the run loop (two node bodies of the degree in a loop; a third one may serve a frame's first sweep in the
     layer loop): per half of the loop unrolled by two everything a wave issues from the head of one node to the head of the other
     (VALU, SALU, branches taken), by the cheapest way that issues the message loads -- once without a barrier, once through one --
     and the register moves and lane accesses it meets between the two node bodies; then what the half waits for (waits_of): the operand
     of the node's first LDS wait, where scalar loads and message loads are issued and how many lie in the next trip's head, the
     vmcnt operands.
 (b) one HAZARD layer of the single-pair lane-chain form (check_node_chain_v2) of that degree: the text between the node's first
     s_setprio 0 and the message packing behind its last phase, split at its two barriers into P1 (regular entries read and reduced,
     heads' pair, chain operands published), walk (per chain: prologue + ONE four-step trip of the walk loop + the three tail steps)
     and P3 (pair completed, minima merged, outputs, packing). This is text in address order: every arm of a lane-divergent branch
     counts once, as every wave with rows of both kinds issues it.
 (c) one trip of the syndrome PRE-TEST (four edges of one layer's 360 checks).
Cycles are per wave at the saturated rates (cycles per wave-instruction per SIMD).
"""
import argparse
import heapq
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from node_census import tally  # noqa: E402
from valu_census import B, RATES, short  # noqa: E402


def disassemble(obj):
    """as node_census.disassemble, with branch targets as labels"""
    with tempfile.TemporaryDirectory() as td:
        fb, elf = os.path.join(td, "k.fatbin"), os.path.join(td, "k.elf")
        subprocess.check_call([B + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
        subprocess.check_call([B + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fb, "--output=" + elf])
        return subprocess.run([B + "llvm-objdump", "-d", "--symbolize-operands", elf], capture_output=True, text=True, check=True).stdout


def blocks_of(dis, want):
    """basic blocks of kernel `want`: list of [ops], label -> block index"""
    ops, labels, name = [], {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            if m.group(1).startswith("_Z"):
                name = short(m.group(1))
            elif name == want:
                labels[m.group(1)] = len(ops)
            continue
        if name != want:
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(//.*)?$", line)
        if m:
            ops.append((m.group(1), m.group(2)))
    starts = set(labels.values()) | {0}
    for i, (o, _) in enumerate(ops):
        if "branch" in o or o == "s_endpgm":
            starts.add(i + 1)
    order = sorted(s for s in starts if s < len(ops))
    blk = [ops[a:b] for a, b in zip(order, order[1:] + [len(ops)])]
    at = {s: k for k, s in enumerate(order)}
    succ = []
    for k, b in enumerate(blk):
        o, a = b[-1]
        s = []
        if "branch" in o:
            s.append(at[labels[a.split()[-1]]])
        if o not in ("s_branch", "s_endpgm") and k + 1 < len(blk):
            s.append(k + 1)
        succ.append(s)
    names = {at[v]: k for k, v in labels.items()}
    return blk, succ, names


def find_nodes(blk, deg):
    """every packed regular node of the degree: [(block, index of its s_setprio 0)]"""
    out = []
    for k in range(len(blk)):
        kk, i = find_node(blk, deg, k)
        if kk == k:
            out.append((k, i))
    return out


def node_form(b, i):
    """"run" / "loop": which form of check_node_v2 the body behind the s_setprio 0 at b[i] is, by its wrap fix -- the run loop's selects the
    base with a v_cndmask_b32 on the record's lane mask, the layer loop's adds under an EXEC mask (s_and_b64 exec). None: neither mark."""
    if any(x == "s_and_b64" and y.startswith("exec") for x, y in b[i:]):
        return "loop"
    return "run" if any(x.startswith("v_cndmask_b32") for x, _ in b) else None


def find_node(blk, deg, first=0):
    """A packed regular node of the degree, by its LLR byte WRITES between s_setprio 0 and the end of its block: `deg` of them in the
    layer loop's form, deg - 1 in the run loop's (the own-parity byte stays in the carry; told from the layer loop's form of the next
    lower degree by node_form). A body with deg - 1 writes and neither mark of a form stops the census: it cannot be told which degree it
    is. (The byte READS no longer tell: without an asm statement in the address phase the scheduler moves some of them in front of the
    s_setprio 0.)"""
    for k, b in enumerate(blk):
        if k < first:
            continue
        for i, (o, a) in enumerate(b):
            if o == "s_setprio" and a.startswith("0"):
                rest = b[i:]
                if not (any(x == "s_setprio" and y.startswith("3") for x, y in rest) and any(x.startswith("v_pk_") for x, _ in rest)) \
                        or any(x == "s_barrier" for x, _ in rest):
                    continue
                writes = sum(1 for x, _ in rest if x.startswith("ds_write_b8"))
                form = node_form(b, i)
                if form is None and writes in (deg - 1, deg):
                    sys.exit(f"block {k}: a packed node with {writes} byte writes and the wrap fix of neither form")
                if writes == (deg - 1 if form == "run" else deg):
                    return k, i
    return None, None


def cheapest_cycle(blk, succ, k0):
    """cheapest cycle (instructions) through block k0 that loads messages, stores messages and meets no barrier"""
    bar = [any(o == "s_barrier" for o, _ in b) for b in blk]
    ld = [any(o.startswith("buffer_load") for o, _ in b) for b in blk]
    st = [any(o.startswith("buffer_store") for o, _ in b) for b in blk]
    f0 = (ld[k0], st[k0])
    dist, prev, heap = {}, {}, [(0, s, f0, (k0, f0)) for s in succ[k0]]
    goal = None
    while heap:
        d, k, f, p = heapq.heappop(heap)
        if (k, f) in dist or (bar[k] and k != k0):
            continue
        dist[(k, f)], prev[(k, f)] = d, p
        if k == k0:
            if f == (True, True):
                goal = (k, f)
                break
            continue
        g = (f[0] or ld[k], f[1] or st[k])
        for s in succ[k]:
            heapq.heappush(heap, (d + len(blk[k]), s, g, (k, f)))
    if goal is None:
        return None
    path, n = [], prev[goal]
    while n != (k0, f0):
        path.append(n[0])
        n = prev[n]
    return path[::-1]


def cheapest_path(blk, succ, src, i_src, dst, i_dst, barrier=False):
    """cheapest way (instructions) from the end of block src to the head of block dst that issues message loads (a buffer_load in the
    node's own block behind its head at i_src, in a block on the way, or in dst in front of its node's head at i_dst: the way of every sweep
    but a frame's first) and meets no barrier -- or, with `barrier`, at least one: [blocks between them]"""
    # (the sweep is wave-uniform code with EXEC restored behind every masked add: the compiler's guards "s_cbranch_execz" around the
    # hand-over blocks at a run's end are never taken, "s_cbranch_execnz" always -- without this the cheapest way leads through them)
    def live(k):
        o = blk[k][-1][0]
        return succ[k][1:] if o == "s_cbranch_execz" and len(succ[k]) == 2 else succ[k][:1] if o == "s_cbranch_execnz" else succ[k]
    bar = [any(o == "s_barrier" for o, _ in b) for b in blk]
    ld = [any(o.startswith("buffer_load") for o, _ in b) for b in blk]
    ld_src = any(o.startswith("buffer_load") for o, _ in blk[src][i_src:])
    ld_dst = any(o.startswith("buffer_load") for o, _ in blk[dst][:i_dst])
    bar_dst = any(o == "s_barrier" for o, _ in blk[dst][:i_dst])
    start = (src, ld_src, False)
    dist, prev, heap = {}, {}, [(0, (s, ld_src, False), start) for s in live(src)]
    while heap:
        d, n, p = heapq.heappop(heap)
        k, l, b = n
        if k == dst:
            l, b = l or ld_dst, b or bar_dst
            if l and b == barrier:
                path = []
                while p != start:
                    path.append(p[0])
                    p = prev[p]
                return path[::-1]
            continue
        if n in dist or (bar[k] and not barrier):
            continue
        dist[n], prev[n] = d, p
        for s in live(k):
            heapq.heappush(heap, (d + len(blk[k]), (s, l or ld[k], b or bar[k]), n))
    return None


def run_loop_pair(blk, succ, nodes):
    """the two node bodies of the run loop among the packed regular nodes of the degree: the pair with the shortest way round (a build may
    keep a third body in the layer loop, for a frame's first sweep)"""
    best = None
    for x in range(len(nodes)):
        for y in range(x + 1, len(nodes)):
            (ka, ia), (kb, ib) = nodes[x], nodes[y]
            ab, ba = cheapest_path(blk, succ, ka, ia, kb, ib), cheapest_path(blk, succ, kb, ib, ka, ia)
            if ab is None or ba is None:
                continue
            n = sum(len(blk[k]) for k in ab + ba)
            if best is None or n < best[0]:
                best = (n, [nodes[x], nodes[y]])
    return best[1] if best else None


def taken(seq):
    """branches TAKEN along a sequence of blocks: transitions that are not a fall-through into the next block in address order"""
    return sum(1 for a, b in zip(seq, seq[1:]) if b != a + 1)


def row(name, c):
    return (f"{name:22s} {c['valu']:5d} {c['full']:5d} {c['half']:5d} {c['quarter']:5d} {c['lds']:4d} {c['salu']:5d} {c['cycles']:8.1f}")


def span_tally(ops):
    c = tally(ops)
    c["vmem"] = sum(1 for o, _ in ops if o.startswith("buffer_"))
    return c


def waits_of(ops):
    """what a half of the run loop waits for, from the head of its node (ops[0], the s_setprio 0) to the head of the other one. A trip's head
    is what lies between the message store of the trip before and its node's head, so the span holds this node and the NEXT trip's head:
    the node's first LDS wait with its operand (scalar loads share lgkmcnt with the byte reads and return out of order: one of them in
    flight makes that wait lgkmcnt(0) and puts a scalar-cache round trip under it), where the scalar loads and the message loads are
    issued, in instructions from the node's head, how many of each lie in the next trip's head, and every vmcnt operand on the way"""
    first = next((i for i, (o, a) in enumerate(ops) if o == "s_waitcnt" and "lgkmcnt" in a), None)
    store = max((i for i, (o, _) in enumerate(ops) if o.startswith("buffer_store")), default=len(ops))
    sl = [i for i, (o, _) in enumerate(ops) if o.startswith("s_load")]
    bl = [i for i, (o, _) in enumerate(ops) if o.startswith("buffer_load")]
    vm = [re.search(r"vmcnt\((\d+)\)", a).group(0) for o, a in ops if o == "s_waitcnt" and "vmcnt" in a]
    return (f"node's first LDS wait: {ops[first][1] if first is not None else 'none'} at {first}; s_load at {sl or 'none'}, buffer_load at {bl or 'none'}, "
            f"message store at {store} of {len(ops)} instructions from the node's head; in the next trip's head (behind the store): "
            f"{sum(1 for i in sl if i > store)} s_load, {sum(1 for i in bl if i > store)} buffer_load; vmcnt waits: {' '.join(vm) or 'none'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj", default=os.path.join(ROOT, "gr-dvbs2rx_amd", "build", "ldpc_inst_8.o"))
    ap.add_argument("--kernel", default="ldpc_layered_kernel<8, packed, solo>")
    ap.add_argument("--deg", type=int, default=7)
    a = ap.parse_args()
    blk, succ, names = blocks_of(disassemble(a.obj), a.kernel)
    if not blk:
        sys.exit(f"{a.kernel} not found in {a.obj}")
    print(f"{a.kernel}  ({os.path.relpath(a.obj, ROOT)}; rates {RATES})")
    print(f"{'part':22s} {'valu':>5} {'full':>5} {'half':>5} {'quart':>5} {'lds':>4} {'salu':>5} {'cycles':>8}")
    # (a)
    k0, i0 = find_node(blk, a.deg)
    if k0 is None:
        sys.exit(f"no packed regular node of degree {a.deg}")
    path = cheapest_cycle(blk, succ, k0)
    if path is None:
        sys.exit("no cycle through the node")
    node = span_tally(blk[k0][i0:])
    rest_ops = blk[k0][:i0] + [op for k in path for op in blk[k]]
    rest = span_tally(rest_ops)
    print(f"(a) regular layer trip, degree {a.deg}; blocks " + " ".join(names.get(k, f"+{k}") for k in [k0] + path))
    print(row("  node + packing", node))
    print(row("  else", rest))
    print("      else VALU: " + " ".join(o for o, _ in rest_ops if o.startswith("v_")))
    print(f"      else: {rest['vmem']} buffer instructions, {sum(1 for o, _ in rest_ops if o == 's_waitcnt')} s_waitcnt")
    # (a') the run loop (degree classes up to 8): the node is instantiated twice per degree, one body per half of the loop unrolled by two
    # over ping-pong record registers; a trip is one node and the way to the other one (the cheapest one: no barrier, not a frame's first sweep)
    found = find_nodes(blk, a.deg)
    forms = [node_form(blk[k], i) for k, i in found]
    print(f"      bodies of degree {a.deg}: " + ", ".join(f"{names.get(k, f'+{k}')} ({f})" for (k, _), f in zip(found, forms)))
    nodes = run_loop_pair(blk, succ, found) if len(found) >= 2 else None
    # the run loop has exactly two bodies of a degree, and they are the pair with the shortest way round: anything else is a misreading
    run_bodies = [n for n, f in zip(found, forms) if f == "run"]
    if run_bodies and (len(run_bodies) != 2 or nodes is None or sorted(nodes) != sorted(run_bodies)):
        sys.exit(f"run-loop bodies of degree {a.deg}: found {len(run_bodies)} in the run form, the loop pair is {nodes}")
    if nodes:
        print(f"(a') run loop, degree {a.deg}: two halves (node -> way to the other node through the message loads; +bar: the way through a barrier)")
        for h, ((ka, ia), (kb, ib)) in enumerate((nodes, nodes[::-1])):
            for barrier in (False, True):
                way = cheapest_path(blk, succ, ka, ia, kb, ib, barrier)
                tag = f"  half {'AB'[h]}" + (" +bar" if barrier else "")
                if way is None:
                    print(f"{tag}: no such way from {names.get(ka, ka)} to {names.get(kb, kb)}")
                    continue
                ops = blk[ka][ia:] + [op for k in way for op in blk[k]] + blk[kb][:ib]
                c = span_tally(ops)
                moves = [f"{o} {x}" for o, x in ops[len(blk[ka][ia:]):] if o.startswith(("v_mov_b32", "v_readfirstlane", "v_readlane", "v_writelane"))]
                print(row(tag, c) + f"   branches taken {taken([ka] + way + [kb])}, {c['vmem']} buffer instructions, "
                      f"{sum(1 for o, _ in ops if o == 's_waitcnt')} s_waitcnt; blocks " + " ".join(names.get(k, f"+{k}") for k in [ka] + way + [kb]))
                if not barrier:
                    print(f"      moves and lane accesses between the node bodies: {len(moves)}" + ("".join("\n        " + m for m in moves)))
                    print("      " + waits_of(ops))
    # (b) the chain node: two barriers with a float walk (v_med3_f32) between them, DEG - 2 + 3 LLR byte reads in front
    flat = [op for b in blk for op in b]
    bars = [i for i, (o, _) in enumerate(flat) if o == "s_barrier"]
    done = False
    for b0, b1 in zip(bars, bars[1:]):
        if not any(o == "v_med3_f32" for o, _ in flat[b0:b1]):
            continue
        # the node's own s_setprio 0 is the last one in front of its first barrier
        cand = [i for i in range(b0) if flat[i][0] == "s_setprio" and flat[i][1].startswith("0")]
        if not cand:
            continue
        p = max(cand)
        if sum(1 for o, _ in flat[p:b0] if o == "ds_read_u8") != a.deg + 1:
            continue
        e = next(i for i in range(b1, len(flat)) if flat[i][0] == "s_setprio" and flat[i][1].startswith("3"))
        while "branch" not in flat[e][0] and flat[e][0] != "s_waitcnt":
            e += 1
        print(f"(b) hazard layer, single-pair lane chain, degree {a.deg} (text in address order)")
        print(row("  P1", span_tally(flat[p:b0])))
        print(row("  walk", span_tally(flat[b0 + 1:b1])))
        print(row("  P3", span_tally(flat[b1 + 1:e])))
        done = True
        break
    if not done:
        print(f"(b) no single-pair lane-chain node of degree {a.deg} in this kernel")
    # (c) the pre-test loop: one block that branches back to itself, with four LLR byte reads
    for k, b in enumerate(blk):
        if k in succ[k] and sum(1 for o, _ in b if o == "ds_read_u8") == 4 and not any(o.startswith("v_pk_") for o, _ in b):
            print("(c) syndrome pre-test trip (four edges)")
            print(row("  trip", span_tally(b)))
            break
    else:
        print("(c) pre-test loop not found as a single block")


if __name__ == "__main__":
    main()
