"""CPU: the routing table of bgn_amd/csrc/dispatch.hpp — which kernel family serves (work, count) and how a large batch
is cut — for every limb count, with and without the table walk, under the defaults, every setting of the GPU tests'
force helpers, the single options and calibrated crossovers.  tests/cpp/dispatch_test.cpp prints one line per
configuration and work with its cases behind it (count, family letter, head where the batch is cut), built with the
address and undefined-behaviour sanitizers; tests/golden/dispatch_routes.txt is what the nine routing functions
that engine.cpp had before the header gave for the same cases (launcher refusals included), so the header must route
exactly as they did.  The GPU tests that force a family and read last_kernel_name() check the launches themselves."""
import os
import subprocess

from conftest import ROOT

# The one behaviour that changed with the header: makeL2 at 3 limbs (no lane-group instantiation) with quad_max_l2 and
# quad_min forced used to land on the lane kernel after the refused lane-group launch; like Mult and Decrypt it now
# skips the missing family and takes the cooperative kernel within its limit (2048).  fixture line -> line now
_TAIL = " 2049L 20000L 20001L 65537L/65536 70000L/65536 1048576L 1049576L/1048576 4194304L"
CHANGED = {
    "3 1 quad_max_l2=20000,quad_min=0 MakeL2: 1L 2048L" + _TAIL: "3 1 quad_max_l2=20000,quad_min=0 MakeL2: 1C 2048C" + _TAIL,
}


def test_routing_table_matches_the_recorded_one():
    src = os.path.join(ROOT, "tests", "cpp", "dispatch_test.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "_build", "dispatch_test")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_routes.txt")) as f:
        want = f.read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want) and len(want) == 6 * 17 * (2 * 4 + 2)
    changed = 0
    for w, g in zip(want, got):
        if w != g:
            assert CHANGED.get(w) == g, f"recorded: {w!r}, now: {g!r}"
            changed += 1
    assert changed == len(CHANGED)
    for work in ("Mult", "MakeL2", "Lift", "Power"):
        for fam in ("Lane", "Coop", "Quad"):
            assert any(f" {work}:" in g and any(t.split("/")[0].endswith(fam[0]) for t in g.split(": ")[1].split()) for g in got), (work, fam)


def test_dispatch_header_is_host_only():
    with open(os.path.join(ROOT, "bgn_amd", "csrc", "dispatch.hpp")) as f:
        text = f.read()
    assert "getenv" not in text
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i == '"options.hpp"' or (i.startswith("<") and "/" not in i and "hip" not in i) for i in includes), includes
