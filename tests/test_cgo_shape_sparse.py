"""bgn_sparse_lincomb_batch / _dev from plain C in the call shape of go/bgn_amd.go (tests/cpp/cgo_shape_sparse.c, gcc
-std=c99): without a GPU it builds, links and fails loudly; with one every form returns the oracle's results for the
ragged structure of test_gpu_sparse_lincomb.py, deterministic and blinded."""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_fixture
from test_cgo_shape_sum import h

BIN = os.path.join(ROOT, "tests", "cpp", "_build", "cgo_shape_sparse")


def run(fx, *args):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "bgn_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cgo_shape_sparse.c"),
                           "-L" + lib, "-lbgn_amd", "-Wl,-rpath," + lib, "-o", BIN])
    return subprocess.run([BIN, h(fx["p"]), h(fx["n"]), str(fx["l"]), fx["P"], fx["Q"]] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=120)


def test_the_c_caller_builds_and_fails_loudly_without_gpu():
    import torch
    fx = load_fixture("toy64")
    E = 2 * fx["fp_bytes"]
    r = run(fx, 1, 1, 1, 1, 1, 7, "00" * E, "00" * 16, "00" * E, "00" * 8, "00" * E)
    assert torch.cuda.is_available() or (r.returncode == 3 and "no HIP device" in r.stdout), r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
def test_c_caller_gets_the_oracles_results(level):
    from test_gpu_sparse_lincomb import material, problem
    m = material("toy64")
    o, n = m.o, m.n
    s, ct, want, totals = problem(m, level, "ragged", 7, "cgo-sparse-%d" % level)
    rng = random.Random("cgo-sparse-r-%d" % level)
    rs = [rng.randrange(n) for _ in totals]
    if level == 1:
        want_b = o.encrypt([t[0] for t in totals], [(t[1] + r) % n for t, r in zip(totals, rs)])
    else:
        Q = bytes.fromhex(m.fx["Q"])
        want_b = o.add(2, want, o.multconst(2, o.mult(Q, Q) * len(rs), rs))
    idx = np.concatenate([s["rp"], s["col"], s["w"]]).astype(np.int64).astype(np.uint32).tobytes()
    rb = b"".join(r.to_bytes((n.bit_length() + 7) // 8, "big") for r in rs)
    r = run(m.fx, level, s["d"], len(s["rp"]) - 1, len(s["col"]), s["row_max"], 7, ct.hex(), idx.hex(), want.hex(), rb.hex(),
            want_b.hex())
    assert r.returncode == 0 and "%d results, 0 failures" % len(totals) in r.stdout, r.stdout + r.stderr
