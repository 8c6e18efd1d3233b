"""The compressed-form entry points of the C ABI from plain C, in the call shape of go/bgn_amd.go's CompressBatch,
DecompressBatch and their Dev forms: tests/cpp/cgo_shape_compress.c is compiled with gcc -std=c99 against
include/bgn_amd.h — on the CPU it must build, link and fail loudly without a GPU; on the GPU every form returns the
bytes Python integers give (handed in from here)."""
import os
import subprocess

import pytest

from conftest import ROOT, load_fixture

BIN = os.path.join(ROOT, "tests", "cpp", "_build", "cgo_shape_compress")


def build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "bgn_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cgo_shape_compress.c"),
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
    L = fx["fp_bytes"]
    r = subprocess.run(_key(fx) + ["1", "00" * (2 * L), "00" * (L + 1)], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["toy64", "k256"])
def test_c_caller_gets_the_reference_bytes(name, level):
    from test_gpu_compress import inputs, ref_compress
    build()
    eng, p, L, rows = inputs(name, level)
    rows = rows[:2] + rows[3:9]                           # (canonical residues: the round trip is the identity)
    want = b"".join(ref_compress(level, r, p, L) for r in rows)
    r = subprocess.run(_key(load_fixture(name)) + [str(level), b"".join(rows).hex(), want.hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "%d elements, 0 failures" % len(rows) in r.stdout, r.stdout + r.stderr
