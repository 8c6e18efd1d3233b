"""CPU: the planning of segmented sums (bgn_amd/csrc/dispatch.hpp plan_sum) — tests/cpp/sum_plan_test.cpp, built with
the address and undefined-behaviour sanitizers as a stand-alone program: the passes terminate, split <= length at every
pass, a forced first split is honoured, and split * ceil(len / split) covers every element exactly once."""
import os
import subprocess

from conftest import ROOT


def test_the_planner_holds_its_properties():
    src = os.path.join(ROOT, "tests", "cpp", "sum_plan_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "_build", "sum_plan_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    assert "1 x 1048576: 65536" in r.stdout and "65536 x 16: 1" in lines


def test_the_options_exist():
    with open(os.path.join(ROOT, "bgn_amd", "csrc", "options.hpp")) as f:
        text = f.read()
    for name in ("sum_split", "sum_run_min"):
        assert '{"%s", &Options::%s, true, nullptr}' % (name, name) in text
