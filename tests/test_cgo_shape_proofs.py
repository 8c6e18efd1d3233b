"""The proof entry points of the C ABI from plain C, in the call shape of go/bgn_amd.go's new methods:
tests/cpp/cgo_shape_proofs.c is compiled with gcc -std=c99 against include/bgn_amd.h — on the CPU it must build, link
and fail loudly without a GPU; on the GPU Prove / Challenge / Verify through host buffers and through device arrays
return the bytes of the Python mirror."""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_fixture

BIN = os.path.join(ROOT, "tests", "cpp", "_build", "cgo_shape_proofs")


def build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "bgn_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cgo_shape_proofs.c"),
                           "-L" + lib, "-lbgn_amd", "-Wl,-rpath," + lib, "-o", BIN])


def h(s):
    s = s[2:] if s.startswith("0x") else s
    return s if len(s) % 2 == 0 else "0" + s


def test_the_c_caller_builds_and_fails_loudly_without_gpu():
    import torch
    build()
    if torch.cuda.is_available():
        return                                            # (with a GPU the gpu test below runs the program)
    fx = load_fixture("toy64")
    n_len = (int(fx["n"], 16).bit_length() + 7) // 8
    s, e = "00" * n_len, "00" * (2 * fx["fp_bytes"])
    r = subprocess.run([BIN, h(fx["p"]), h(fx["n"]), str(fx["l"]), fx["P"], fx["Q"], s, s, s, s, e, e, s, "00" * 32],
                       capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_c_caller_proves_and_verifies_like_the_mirror():
    import bgn_amd
    import bgn_ref as R
    build()
    opk, osk = R.NewKeyGen(128, 1021, 3, True, 133)        # (a generated key carries R; the fixtures do not)
    p, n = opk.p, opk.n
    Pw, Qw = R.elem_to_bytes(opk.P, p), R.elem_to_bytes(opk.Q, p)
    pk = bgn_amd.PublicKey(p, n, opk.l, Pw, Qw, 1021)
    sk = bgn_amd.SecretKey(osk.Key, osk.R)
    rng = random.Random(12)
    nl = pk.engine.n_len
    count = 5
    vs, zs, ns = ([rng.randrange(n) for _ in range(count)] for _ in range(3))
    proofs = pk.NewProofOfPlaintextKnowledgeBatch(sk, vs, zs, ns)
    assert pk.CheckProofOfPlaintextKnoewledgeBatch([pr.Ct for pr in proofs], proofs) == [True] * count
    rq = sk.R * (n // sk.Key) % n
    pack = lambda xs: b"".join(x.to_bytes(nl, "big") for x in xs).hex()
    want_c = b"".join(hashlib.sha256(pr.Ct.C + pr.Nonce.C).digest() for pr in proofs).hex()
    r = subprocess.run([BIN, h(hex(p)), h(hex(n)), str(opk.l), Pw.hex(), Qw.hex(), pack(vs), pack(zs), pack(ns), pack([rq]),
                        b"".join(pr.Ct.C for pr in proofs).hex(), b"".join(pr.Nonce.C for pr in proofs).hex(),
                        pack([pr.DL for pr in proofs]), want_c], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "5 proofs, 0 failures" in r.stdout, r.stdout + r.stderr
