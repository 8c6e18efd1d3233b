"""CPU: the seeded expansion of blinding scalars (csrc/randexp.hpp, "expansion 1" of include/bgn_amd.h) on the host
emulation of the device headers, against hashlib and Python's % (tests/randexp_oracle.py): rand_block, rand_reduce and
the whole scalar, the latter two with the range checks on (a failed check aborts).

Every fixture key ends W inside a block (n_len + 16 = 16 or 24 mod 32), so the moduli under test are the fixture
orders AND, per instantiation, an odd modulus whose W ends on a block boundary (n_len = 16 mod 32) and one of the
longest n_len the instantiation serves."""
import ctypes as C
import glob
import os
import random
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_fixture

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import emu  # noqa: E402
import randexp_oracle as X  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(ROOT, "bgn_amd", "csrc")
_SRC = os.path.join(_HERE, "emu_randexp.cpp")
_SO = os.path.join(_EMU, "_build", "libbgn_emu_randexp.so")

FIXTURES = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(GOLDEN, "*.json")))
KEYS = [k for k in FIXTURES if "p" in load_fixture(k) and "n" in load_fixture(k)]
EDGE = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]


def _build():
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("randexp.hpp", "sha256.hpp", "proofs.hpp", "fpmont.hpp", "codec.hpp",
                                                      "consts.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-rdynamic", "-std=c++17", "-fPIC", "-shared", "-I" + _EMU, "-I" + _CSRC,
                               "-include", os.path.join(_EMU, "agpr.hpp"), "-include", os.path.join(_EMU, "gmem.hpp"),
                               "-include", os.path.join(_EMU, "imad.hpp"), _SRC, "-o", _SO])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def lib():
    return _build()


def _words(K: bytes):
    return (C.c_uint32 * 8)(*[int.from_bytes(K[4 * m:4 * m + 4], "big") for m in range(8)])


# ---- rand_block ------------------------------------------------------------------------------------------------------
def test_rand_block_matches_hashlib(lib):
    """Random seeds (and the all-zero and all-ones ones), t and i at 0, 1, 2^32 - 1, 2^32, 2^64 - 1, j at 0, 1, 4."""
    rng = random.Random(9)
    out = C.create_string_buffer(32)
    for K in [bytes(32), b"\xff" * 32] + [rng.randbytes(32) for _ in range(6)]:
        for t in EDGE:
            for i in EDGE:
                for j in (0, 1, 4):
                    lib.randexp_block(_words(K), C.c_uint64(t), C.c_uint64(i), C.c_uint32(j), out)
                    assert out.raw == X.block(K, t, i, j), (K.hex(), t, i, j)


# ---- the moduli ------------------------------------------------------------------------------------------------------
class Order:
    """The parameter block of a modulus n at nl limbs, as engine.cpp builds it (build_params(n, nl))."""

    def __init__(self, n: int, nl: int):
        self.n, self.nl, self.n_len = n, nl, X.n_len_of(n)
        R = 1 << (emu.LIMB * nl)
        img = emu.limbs(n, nl) + emu.limbs(R % n, nl) + emu.limbs(R * R % n, nl)
        for K in range(1, emu.KP_MAX + 1):
            img += emu.limbs(K * n, nl)
        img += [(-pow(n, -1, 1 << emu.LIMB)) % (1 << emu.LIMB), 0, 0, 0]
        self.params = (C.c_uint32 * len(img))(*img)

    def reduce(self, lib, w: int) -> int:
        wl = lib.randexp_w_limbs(self.nl)
        assert w < 1 << (8 * (self.n_len + X.SURPLUS)) <= 1 << (emu.LIMB * wl)
        out = (C.c_uint32 * self.nl)()
        assert lib.randexp_reduce(self.nl, self.params, (C.c_uint32 * wl)(*emu.limbs(w, wl)), out) == 0
        return sum(int(v) << (emu.LIMB * j) for j, v in enumerate(out))

    def scalar(self, lib, K: bytes, t: int, i: int) -> int:
        out = C.create_string_buffer(self.n_len)
        assert lib.randexp_scalar(self.nl, self.params, self.n_len, _words(K), C.c_uint64(t), C.c_uint64(i), out) == 0
        return int.from_bytes(out.raw, "big")


def _fixture_order(name):
    fx = load_fixture(name)
    return Order(int(fx["n"], 16), emu.nl_for(int(fx["p"], 16)))


def _odd(rng, n_len):
    return rng.getrandbits(8 * n_len) | (1 << (8 * n_len - 1)) | 1


# (nl, n_len): W ends on a block boundary / the longest order of the instantiation, (LIMB * nl - 2) // 8 bytes
SYNTHETIC = [(10, 16), (19, 48), (36, 112), (37, 112), (72, 240), (3, 10), (10, 36), (19, 68), (36, 130), (37, 133), (72, 260)]
CASES = [("fixture", k) for k in KEYS] + [("synthetic", s) for s in SYNTHETIC]


def _order(kind, what):
    if kind == "fixture":
        return _fixture_order(what)
    nl, n_len = what
    return Order(_odd(random.Random(1000 * nl + n_len), n_len), nl)


def test_the_moduli_cover_every_instantiation_and_both_ends_of_w(lib):
    orders = [_order(*c) for c in CASES]
    assert {o.nl for o in orders if o.n in [_fixture_order(k).n for k in KEYS]} == {3, 10, 19, 36, 37, 72}
    ends = {(o.n_len + X.SURPLUS) % 32 == 0 for o in orders}
    assert ends == {True, False}                      # W ends on a block boundary, and inside a block
    for nl in (3, 10, 19, 36, 37, 72):
        assert lib.randexp_max_n_len(nl) == (emu.LIMB * nl - 2) // 8
        assert max(o.n_len for o in orders if o.nl == nl) == lib.randexp_max_n_len(nl)
    assert all(o.n_len <= lib.randexp_max_n_len(o.nl) for o in orders)
    assert lib.randexp_w_limbs(3) > 2 * 3             # at three limbs W is several pieces long


@pytest.mark.parametrize("kind,what", CASES, ids=[str(c[1]) for c in CASES])
def test_rand_reduce_matches_python_integers(lib, kind, what):
    """W mod n for W of n_len + 16 bytes: random ones, all ones, 0, n - 1, n, n + 1, and k*n, k*n - 1 for the largest k
    that fits."""
    O = _order(kind, what)
    n, top = O.n, 1 << (8 * (O.n_len + X.SURPLUS))
    k = (top - 1) // n
    rng = random.Random(O.nl)
    ws = [top - 1, 0, 1, n - 1, n, n + 1, k * n, k * n - 1, (k - 1) * n + 1, 1 << (8 * (O.n_len + X.SURPLUS) - 1)]
    ws += [rng.randrange(top) for _ in range(60)] + [rng.randrange(1 << 128) * n + rng.choice((0, 1, n - 1)) for _ in range(20)]
    assert k * n < top <= (k + 1) * n
    for w in ws:
        assert O.reduce(lib, w) == w % n, (what, hex(w))


@pytest.mark.parametrize("kind,what", CASES, ids=[str(c[1]) for c in CASES])
def test_the_whole_scalar_matches_the_oracle(lib, kind, what):
    """Blocks, truncation to n_len + 16 bytes and reduction together, for random seeds and the edge values of t and i."""
    O = _order(kind, what)
    rng = random.Random(7 * O.nl + O.n_len)
    for K in [bytes(32)] + [rng.randbytes(32) for _ in range(3)]:
        for t, i in [(t, i) for t in EDGE for i in EDGE][::3] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(8)]:
            got = O.scalar(lib, K, t, i)
            assert got == X.scalar(K, t, i, O.n) and got < O.n, (what, K.hex(), t, i)
