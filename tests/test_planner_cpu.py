"""CPU: the launch planners (csrc/nlspn_plan.h) give the recorded plans.

The GPU parity tests are bit-exact for any part grid, so a change that silently alters a
plan changes speed and fails nothing there.  tests/planner_dump.cpp, a host-only program (no
device, no HIP header), prints res_plan's and br_plan's records for the shapes where the plan
can go wrong; they must equal tests/golden/resident_plans.json, the table recorded from the
planner as it stood when it was one function of the C-ABI unit.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nlspn_eccv20_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "resident_plans.json")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("planner") / "planner_dump")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "planner_dump.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, env={})  # no device, no A/B switch, no Python
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_case_list(plans, golden):
    for kind in ("forward", "backward"):
        assert [r["name"] for r in plans[kind]] == [r["name"] for r in golden[kind]]
    rows = {r["name"]: r for r in golden["forward"]}
    # the table holds the shapes it is meant to: C1 split quads, C3 merged, C5 four groups ...
    assert rows["C1"]["grid"] == [247] and rows["C1"]["split"] == 1
    assert rows["C3"]["merged"] and rows["C3"]["groups"] == 2
    assert rows["C3 B=5"]["launches"] == 2 and rows["C5"]["groups"] == 4
    assert not rows["5x5"]["merged"] and "build_merged" not in rows["5x5"]
    assert not rows["W%4"]["resident"] and not rows["7x7"]["resident"] and not rows["T=1"]["resident"]
    assert rows["T=2"]["resident"] and not rows["C2 first=0"]["first"]
    # every switch row differs from its default row (a planner that ignored the switch would fail)
    assert rows["C1 split=0"]["nt"] == 128 and rows["C1 split=0"]["split"] == 0 and not rows["C1 split=0"]["first"]
    assert not rows["C3 merge=0"]["merged"] and rows["C3 merge=0"]["grid"] == [256, 256]
    assert {r["cus"] for r in golden["forward"]} == {64, 256, 304}


@pytest.mark.parametrize("kind", ["forward", "backward"])
def test_plans_match_table(plans, golden, kind):
    for got, want in zip(plans[kind], golden[kind]):
        assert got == want, (want["name"], {k: (got.get(k), want.get(k)) for k in set(got) | set(want)
                                            if got.get(k) != want.get(k)})


# The per-element backward cases (tests/_bwd_cases.py, tests/test_gpu_backward_elem.py) select the
# backward's forms by shape alone; a planner change must not move them silently.  At the MI355X's
# 256 CUs: what each case is named for.
BWD_FORMS = {
    "res_tiny_parts": ("resident", 120, 1), "res_far": ("resident", 128, 1),
    "res_one_part": ("resident", 1, 3), "res_two_parts": ("resident", 2, 2),
    "res_T2": ("resident", 128, 1), "res_T24": ("resident", 128, 1), "res_odd": ("resident", 84, 1),
    "res_noconf": ("resident", 120, 1), "res_nopreserve": ("resident", 120, 1),
    "res_AS": ("resident", 120, 1), "res_ASS": ("resident", 120, 1), "res_TC": ("resident", 120, 1),
    "steps_split_clip": "steps", "steps_split_manyB": "steps",
    "onepass_longT": "onepass", "onepass_env": "onepass", "k17": "onepass", "k5x5": "onepass", "k7x7": "onepass",
    "noffset": "onepass", "range": ("resident", 128, 1), "nonexact": ("resident", 120, 1),
    "big_compact": ("resident", 64, 1),  # (the compact batch of tests/_big_cases.py; its large batches take the steps)
}


def test_backward_cases_select_their_forms(tmp_path):
    import _bwd_cases as bc
    got = {n: bc.backward_form(n, 256, str(tmp_path)) for n in bc.CASES if bc.CASES[n]["form"] == "fused"}
    assert got == BWD_FORMS, {n: (got.get(n), BWD_FORMS.get(n)) for n in set(got) | set(BWD_FORMS)
                              if got.get(n) != BWD_FORMS.get(n)}
