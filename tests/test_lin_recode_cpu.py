"""CPU: the signed-window recoding of the linear maps' weights (bgn_amd/csrc/linrecode.hpp) and their planning
(dispatch.hpp plan_lincomb) — tests/cpp/lin_recode_test.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_the_recoding_and_the_planner_hold_their_properties():
    src = os.path.join(ROOT, "tests", "cpp", "lin_recode_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "_build", "lin_recode_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.splitlines()[-1] == "ok"


def test_the_options_exist():
    with open(os.path.join(ROOT, "bgn_amd", "csrc", "options.hpp")) as f:
        text = f.read()
    for name in ("lin_window", "lin_split"):
        assert '{"%s", &Options::%s, true, nullptr}' % (name, name) in text
