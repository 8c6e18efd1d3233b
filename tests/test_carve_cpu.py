"""CPU: the workspace planner of bgn_amd/csrc/carve.hpp — carve() runs a layout twice, against null to size the
workspace and against the arena to hand out its arrays.  tests/cpp/carve_test.cpp, built with the address and
undefined-behaviour sanitizers, runs a layout with a conditional member (G1, GT, an F_p row, raw takes of 1 and 257
bytes) at 3 and 36 limbs and strides 64 and 128 over an arena of exactly the size asked for: the sizing pass reports
the carving pass's end, every array is 256-byte aligned inside the arena and apart from the others, and the offsets
are the ones worked out by hand from "every take is rounded up to 256 bytes"."""
import os
import subprocess

from conftest import ROOT


def test_sizing_pass_and_carving_pass_agree():
    src = os.path.join(ROOT, "tests", "cpp", "carve_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "_build", "carve_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    assert r.stdout.split() == ["ok", "8"]


def test_carve_header_is_host_only():
    for name in ("carve.hpp", "soa.hpp"):
        with open(os.path.join(ROOT, "bgn_amd", "csrc", name)) as f:
            includes = [ln.split()[1] for ln in f.read().splitlines() if ln.startswith("#include")]
        assert includes and all(i == '"soa.hpp"' or (i.startswith("<") and "/" not in i and "hip" not in i) for i in includes), includes
