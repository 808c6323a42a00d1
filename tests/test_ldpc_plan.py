"""CPU: the LDPC planner (csrc/ldpc_plan.cpp: build choice and record layout), compiled with the host compiler.

tests/golden/ldpc_plan.json holds, for every table and every override set the GPU tests use, what the constructor of LdpcDecoderHip
decided and laid out BEFORE the planner existed (recorded from that constructor, notes/ldpc_plan_refactor.md): the kernel name or the
error text, dmax, words_per_check, pr_shared_sv, lds_bytes, gsync_on and a truncated sha256 of the per-layer and of the per-(layer,
wave) record words. Identical plans of a table are stored once; "rows" indexes them per override set.
`python tests/test_ldpc_plan.py RECORDER_EXE` prints that file from any program that speaks tests/ldpc_plan_main.cpp's protocol."""
import json
import os
import re
import sys

import pytest

import fec_testlib as T

GOLDEN = os.path.join(T.ROOT, "tests", "golden", "ldpc_plan.json")
FIELDS = ("name", "dmax", "words_per_check", "pr_shared_sv", "lds_bytes", "gsync_on", "recs", "wrecs")
# the override sets of tests/test_ldpc_gpu.py::test_kernel_variant_policy and ::test_both_variants (tests/test_packed_node_edges_gpu.py uses
# the packed-pair and packed-solo sets of VARIANTS)
POLICY_SETS = [
    {"DVBS2_PR_V2": "0"}, {"DVBS2_PR_W1": "0"}, {"DVBS2_PR_W1": "0", "DVBS2_PR_V2": "0"}, {"DVBS2_DENSE": "0", "DVBS2_V2": "0", "DVBS2_SOLO": "0"},
    {"DVBS2_PR": "0", "DVBS2_V2": "0", "DVBS2_SOLO": "0"}, {"DVBS2_PR": "0"}, {"DVBS2_V2": "1", "DVBS2_SOLO": "1"}, {"DVBS2_V2": "0", "DVBS2_SOLO": "0"},
    {"DVBS2_SOFT_BARRIER": "1"}, {"DVBS2_PR": "1"},
]


def override_sets():
    sets = []
    for env in list(T.VARIANTS.values()) + POLICY_SETS:
        if env not in sets:
            sets.append(env)
    return sets


def policy():
    text = open(os.path.join(T.ROOT, "gr-dvbs2rx_amd", "csrc", "ldpc_policy.inc")).read()
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r'\{ "(\w+)", (\d), (\d) \}', text)}


def flat(plan):
    return [plan["error"]] if "error" in plan else [plan[k] for k in FIELDS]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = T.build_ldpc_planner(tmp_path_factory.mktemp("ldpc_plan"))
    return lambda rows: T.run_ldpc_planner(exe, rows)


def test_plans_equal_the_recorded_constructor(planner):
    """Every row of the golden: same decisions, same record words. The format invariants (ldpc_plan_main.cpp, check_format) on each."""
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["tables"]) == 57 and sorted(g["tables"]) == sorted(policy())
    for env in override_sets():
        assert env in g["sets"], env
    rows = [(t, g["sets"][k], e["plans"][i]) for t, e in sorted(g["tables"].items()) for k, i in enumerate(e["rows"])]
    assert len(rows) >= 57 * 12 and len(rows) == 57 * len(g["sets"])
    for (table, env, want), got in zip(rows, planner([r[:2] for r in rows])):
        assert flat(got) == want, (table, env)
        assert got.get("check", "") == "", (table, env, got["check"])


def test_policy(planner):
    """tests/test_ldpc_gpu.py::test_kernel_variant_policy without a GPU: the same assertions on the planner's kernel name."""
    def name(table, **env):
        return planner([(table, env)])[0]["name"]
    pol = policy()
    assert len(pol) == 57

    def expect(table, dmax):
        packed, solo = pol[table]
        solo = solo and dmax <= 16
        return f"ldpc_layered_kernel<{dmax}" + ((", packed, solo>" if packed else ", solo>") if solo else (", packed>" if packed else ">"))
    assert name("S2_TABLE_B4") == expect("S2_TABLE_B4", 8)
    assert name("S2_TABLE_B7") == expect("S2_TABLE_B7", 16)
    assert name("S2_TABLE_B11") == expect("S2_TABLE_B11", 32)
    assert name("S2X_TABLE_B9") == expect("S2X_TABLE_B9", 16)
    assert name("S2_TABLE_C2") == "ldpc_layered_pr_kernel<packed>"
    assert name("S2_TABLE_C2", DVBS2_PR_V2="0") == "ldpc_layered_pr_kernel"
    assert name("S2_TABLE_C1") == "ldpc_layered_pr_kernel<w1>"
    assert name("S2_TABLE_C1", DVBS2_PR_W1="0") == "ldpc_layered_pr_kernel<packed>"
    assert name("S2_TABLE_C1", DVBS2_PR_W1="0", DVBS2_PR_V2="0") == "ldpc_layered_pr_kernel"
    assert name("S2X_TABLE_C9") == "ldpc_layered_pr_kernel<w1>"
    assert name("S2_TABLE_C5") == "ldpc_layered_kernel<12, dense>"
    assert name("S2_TABLE_C5", DVBS2_DENSE="0", DVBS2_V2="0", DVBS2_SOLO="0") == "ldpc_layered_kernel<12>"
    assert name("S2_TABLE_C1", DVBS2_PR="0", DVBS2_V2="0", DVBS2_SOLO="0") == "ldpc_layered_kernel<4>"
    assert name("S2_TABLE_B1") == "ldpc_layered_pr_kernel<w1>"
    assert name("S2X_TABLE_B1") == "ldpc_layered_pr_kernel<w1>"
    assert name("S2_TABLE_B1", DVBS2_PR="0") == expect("S2_TABLE_B1", 4)
    assert name("S2_TABLE_B2") == expect("S2_TABLE_B2", 8)
    assert name("S2_TABLE_B4", DVBS2_V2="1", DVBS2_SOLO="1") == "ldpc_layered_kernel<8, packed, solo>"
    assert name("S2_TABLE_B4", DVBS2_V2="0", DVBS2_SOLO="0") == "ldpc_layered_kernel<8>"
    assert name("S2_TABLE_B11", DVBS2_V2="1", DVBS2_SOLO="1") == "ldpc_layered_kernel<32, packed>"
    assert name("S2X_TABLE_B21") == ("ldpc_layered_kernel<32, packed, soft>" if pol["S2X_TABLE_B21"][0] else "ldpc_layered_kernel<32, soft>")
    assert name("S2_TABLE_C10") == "ldpc_layered_kernel<28, hz2>"
    assert name("S2_TABLE_B9") == expect("S2_TABLE_B9", 24)
    assert name("S2_TABLE_B9", DVBS2_SOFT_BARRIER="1") == expect("S2_TABLE_B9", 24)[:-1] + ", soft>"
    assert name("S2_TABLE_B4", DVBS2_PR="1") == "ldpc_layered_pr_kernel"
    assert name("S2_TABLE_B1", DVBS2_PR="1") == "ldpc_layered_pr_kernel<w1>"


def test_group_stop_and_errors(planner):
    """gsync_on follows the group size and DVBS2_GROUP_SYNC; a table the library does not have is an error text, not a plan."""
    exe_rows = [("S2_TABLE_B4", {}), ("S2_TABLE_B4", {"DVBS2_GROUP_SYNC": "0"}), ("NO_SUCH_TABLE", {})]
    a, b, c = planner(exe_rows)
    assert a["gsync_on"] == 1 and b["gsync_on"] == 0 and {k: a[k] for k in FIELDS if k != "gsync_on"} == {k: b[k] for k in FIELDS if k != "gsync_on"}
    assert c == {"error": "unknown or inconsistent LDPC table"}


if __name__ == "__main__":  # record the golden with the program given (the recorder of notes/ldpc_plan_recorder.patch)
    sets, tables = override_sets(), {}
    for table in sorted(policy()):
        plans, rows = [], []
        for p in T.run_ldpc_planner(sys.argv[1], [(table, env) for env in sets]):
            if flat(p) not in plans:
                plans.append(flat(p))
            rows.append(plans.index(flat(p)))
        tables[table] = {"plans": plans, "rows": rows}
    text = json.dumps({"sets": sets, "tables": tables}, separators=(",", ":"))
    print(text.replace('},"', '},\n"'))
