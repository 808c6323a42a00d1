"""CPU: the chunk plan of the host-buffer entries (csrc/host_plan.h), compiled with the host compiler.

tests/golden/host_plan.json holds plans recorded from the two copies of the plan code that dvbs2_ldpc_decode and the chain's host entry
each carried before host_plan.h existed (a thinned grid: the full one would be megabytes). The invariants the pipeline relies on are
asserted on the whole grid."""
import itertools
import json
import os
import subprocess

import pytest

import fec_testlib as T

NS = [1, 2, 31, 32, 33, 64, 97, 200, 416, 511, 512, 513, 1023, 1024, 1025, 1088, 2048, 4095, 4096, 16384]
GS = [1, 3, 32, 33, 64, 257, 520]  # odd sizes and sizes above the first chunk of 512: `unit` and the clamps of the bounds
HOST_CHUNKS = [0, 2, 32, 66, 4096]
HOST_PLANS = ["", "64", "512,128", "100,"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "host_plan_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(T.ROOT, "tests", "host_plan_main.cpp"), "-o", exe])

    def run(rows):
        text = "".join("%d %d %d %d %d %s\n" % (n, G, locked, syms, hc, hp or "-") for n, G, locked, syms, hc, hp in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(rows)
        return [[tuple(map(int, t.split(":"))) for t in line.split()] for line in lines]
    return run


def check_invariants(row, plan):
    n, G = row[0], row[1]
    unit = G if G % 2 == 0 else 2 * G
    assert plan, row
    nxt = 0
    for f0, nf in plan:
        assert f0 == nxt and nf > 0, (row, plan)  # contiguous from frame 0, no empty chunk
        nxt = f0 + nf
    assert nxt == n, (row, plan)
    assert all(f0 % unit == 0 for f0, _ in plan), (row, plan)  # every boundary but the call's end: whole groups, whole frame pairs


def test_plan_equals_the_recorded_plans(plans):
    with open(os.path.join(T.ROOT, "tests", "golden", "host_plan.json")) as f:
        rows = json.load(f)["rows"]
    assert len(rows) > 200
    for row, plan in zip(rows, plans([r[:6] for r in rows])):
        assert [x for chunk in plan for x in chunk] == row[6], row[:6]
        check_invariants(row, plan)


def test_plan_invariants_on_the_whole_grid(plans):
    rows = [r for r in itertools.product(NS, GS, (0, 1), (0, 1), HOST_CHUNKS, HOST_PLANS)]
    for row, plan in zip(rows, plans(rows)):
        check_invariants(row, plan)

