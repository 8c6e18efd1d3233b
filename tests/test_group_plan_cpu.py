"""CPU: the column groups of bgn_lincomb_batch — the codes and the table recurrence of grprecode.hpp and the planner
(dispatch.hpp plan_lincomb_groups, lin_path) hold their properties — tests/cpp/group_plan_test.cpp, a stand-alone program
built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_the_group_codes_and_planner_hold_their_properties():
    src = os.path.join(ROOT, "tests", "cpp", "group_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "group_plan_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
