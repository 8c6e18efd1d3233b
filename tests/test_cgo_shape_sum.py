"""The segmented-sum entry points of the C ABI from plain C, in the call shape of go/bgn_amd.go's SumBatch and
SumBatchDev: tests/cpp/cgo_shape_sum.c is compiled with gcc -std=c99 against include/bgn_amd.h — on the CPU it must
build, link and fail loudly without a GPU; on the GPU every form returns the sums the C oracle gives for the exponent
totals of the segments (handed in from here), deterministic and blinded."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_fixture

BIN = os.path.join(ROOT, "tests", "cpp", "_build", "cgo_shape_sum")


def build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "bgn_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cgo_shape_sum.c"),
                           "-L" + lib, "-lbgn_amd", "-Wl,-rpath," + lib, "-o", BIN])


def h(s):
    s = s[2:] if s.startswith("0x") else s
    return s if len(s) % 2 == 0 else "0" + s


def _key(fx):
    return [BIN, h(fx["p"]), h(fx["n"]), str(fx["l"]), fx["P"], fx["Q"]]


def test_the_c_caller_builds_and_fails_loudly_without_gpu():
    import torch
    build()
    if torch.cuda.is_available():
        return                                            # (with a GPU the gpu test below runs the program)
    fx = load_fixture("toy64")
    E = 2 * fx["fp_bytes"]
    r = subprocess.run(_key(fx) + ["1", "2", "00" * (2 * E), "00" * E, "00" * 8, "00" * E], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["toy64", "k256"])
def test_c_caller_gets_the_oracles_sums(name, level):
    import oracle_c
    build()
    fx = load_fixture(name)
    o = oracle_c.Oracle.from_fixture(fx)
    n = int(fx["n"], 16)
    n_len = (n.bit_length() + 7) // 8
    rng = random.Random("cgo-sum-%s-%d" % (name, level))
    nseg, seg_len = 5, 13
    rs = [rng.randrange(n) for _ in range(nseg)]
    if level == 1:
        pool = [(0, 0), (1, 0), (2, 0), (n - 1, 0), (n - 2, 0), (rng.randrange(n), rng.randrange(n))]
        idx = [[rng.randrange(len(pool)) for _ in range(seg_len)] for _ in range(nseg)]
        flat = [pool[i] for row in idx for i in row]
        ct = o.encrypt([e[0] for e in flat], [e[1] for e in flat])
        tx = [sum(pool[i][0] for i in row) % n for row in idx]
        tr = [sum(pool[i][1] for i in row) % n for row in idx]
        want = o.encrypt(tx, tr)
        want_b = o.encrypt(tx, [(a + b) % n for a, b in zip(tr, rs)])
    else:
        one = o.encrypt([1])
        g = o.mult(one, one)
        ks = [0, 1, 2, n - 1]
        pool = o.multconst(2, g * len(ks), ks)
        idx = [[rng.randrange(len(ks)) for _ in range(seg_len)] for _ in range(nseg)]
        ct = b"".join(pool[i * o.E:(i + 1) * o.E] for row in idx for i in row)
        want = o.multconst(2, g * nseg, [sum(ks[i] for i in row) % n for row in idx])
        Q = bytes.fromhex(fx["Q"])
        want_b = o.add(2, want, o.multconst(2, o.mult(Q, Q) * nseg, rs))
    rb = b"".join(r.to_bytes(n_len, "big") for r in rs)
    r = subprocess.run(_key(fx) + [str(level), str(seg_len), ct.hex(), want.hex(), rb.hex(), want_b.hex()],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "%d sums, 0 failures" % nseg in r.stdout, r.stdout + r.stderr
