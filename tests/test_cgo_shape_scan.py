"""bgn_scan_batch / bgn_scan_batch_dev from plain C in the call shape of go/bgn_amd.go (tests/cpp/cgo_shape_scan.c, gcc
-std=c99): without a GPU it builds, links and fails loudly; with one every form returns the oracle's prefixes."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_fixture
from test_cgo_shape_sum import h

BIN = os.path.join(ROOT, "tests", "cpp", "_build", "cgo_shape_scan")


def run(fx, *args):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "bgn_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cgo_shape_scan.c"),
                           "-L" + lib, "-lbgn_amd", "-Wl,-rpath," + lib, "-o", BIN])
    return subprocess.run([BIN, h(fx["p"]), h(fx["n"]), str(fx["l"]), fx["P"], fx["Q"]] + list(args),
                          capture_output=True, text=True, timeout=120)


def test_the_c_caller_builds_and_fails_loudly_without_gpu():
    import torch
    fx = load_fixture("toy64")
    E = 2 * fx["fp_bytes"]
    r = run(fx, "1", "2", "00" * (2 * E), "00" * (2 * E), "00" * 16, "00" * (2 * E))
    assert torch.cuda.is_available() or (r.returncode == 3 and "no HIP device" in r.stdout), r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
def test_c_caller_gets_the_oracles_prefixes(level):
    import oracle_c
    fx = load_fixture("toy64")
    o = oracle_c.Oracle.from_fixture(fx)
    n = int(fx["n"], 16)
    rng = random.Random("cgo-scan-%d" % level)
    seg_len, ks = 13, [0, 1, 2, n - 1]
    idx = [[rng.randrange(len(ks)) for _ in range(seg_len)] for _ in range(3)]
    run_ = [sum(ks[i] for i in row[:j + 1]) % n for row in idx for j in range(seg_len)]
    rs = [rng.randrange(n) for _ in run_]
    if level == 1:
        ct = o.encrypt([ks[i] for row in idx for i in row], [0] * len(run_))
        want, want_b = o.encrypt(run_, [0] * len(run_)), o.encrypt(run_, rs)
    else:
        one = o.encrypt([1])
        g = o.mult(one, one)
        pool = o.multconst(2, g * len(ks), ks)
        ct = b"".join(pool[i * o.E:(i + 1) * o.E] for row in idx for i in row)
        want = o.multconst(2, g * len(run_), run_)
        Q = bytes.fromhex(fx["Q"])
        want_b = o.add(2, want, o.multconst(2, o.mult(Q, Q) * len(run_), rs))
    rb = b"".join(r.to_bytes((n.bit_length() + 7) // 8, "big") for r in rs)
    r = run(fx, str(level), str(seg_len), ct.hex(), want.hex(), rb.hex(), want_b.hex())
    assert r.returncode == 0 and "%d prefixes, 0 failures" % len(run_) in r.stdout, r.stdout + r.stderr
