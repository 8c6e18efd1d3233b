"""The seeded-randomness entry points of the C ABI from plain C, in the call shape of go/bgn_amd.go's new methods:
tests/cpp/cgo_shape_random.c is compiled with gcc -std=c99 against include/bgn_amd.h — on the CPU it must build, link
and fail loudly without a GPU; on the GPU the rows of every form equal the bytes hashlib and Python integers give
(tests/randexp_oracle.py), handed in from here, and the seeded Encrypt equals bgn_encrypt_batch of those rows."""
import os
import random
import subprocess

import pytest

import randexp_oracle as X
from conftest import ROOT, load_fixture

BIN = os.path.join(ROOT, "tests", "cpp", "_build", "cgo_shape_random")


def build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "bgn_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cgo_shape_random.c"),
                           "-L" + lib, "-lbgn_amd", "-Wl,-rpath," + lib, "-o", BIN])


def h(s):
    s = s[2:] if s.startswith("0x") else s
    return s if len(s) % 2 == 0 else "0" + s


def _args(fx, seed, t, first, xs):
    n = int(fx["n"], 16)
    return [BIN, h(fx["p"]), h(fx["n"]), str(fx["l"]), fx["P"], fx["Q"], seed.hex(), str(t), str(first),
            b"".join(x.to_bytes(8, "big") for x in xs).hex(), X.rows(seed, t, first, len(xs), n).hex()]


def test_the_c_caller_builds_and_fails_loudly_without_gpu():
    import torch
    build()
    if torch.cuda.is_available():
        return                                            # (with a GPU the gpu test below runs the program)
    r = subprocess.run(_args(load_fixture("toy64"), bytes(32), 0, 0, [1, 2]), capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy64", "k256"])
def test_c_caller_gets_the_oracles_rows(name):
    build()
    rng = random.Random(31)
    xs = [rng.randrange(1 << 40) for _ in range(67)]
    first = (1 << 32) - 30                                # the rows straddle 2^32
    r = subprocess.run(_args(load_fixture(name), rng.randbytes(32), (5 << 32) | 1, first, xs), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "67 rows, 0 failures" in r.stdout, r.stdout + r.stderr
