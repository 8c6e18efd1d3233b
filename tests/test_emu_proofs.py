"""CPU: the two device functions behind the proofs of plaintext knowledge on the host emulation of the device headers —
sha256_wire (csrc/sha256.hpp) against hashlib at every length and start alignment, and the response modulo the group
order (csrc/proofs.hpp pok_response_bytes) against Python integers with the range checks on (a failed check aborts)."""
import ctypes as C
import glob
import hashlib
import os
import random
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_fixture

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import emu  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(ROOT, "bgn_amd", "csrc")
_SRC = os.path.join(_HERE, "emu_proofs.cpp")
_SO = os.path.join(_EMU, "_build", "libbgn_emu_proofs.so")

FIXTURES = sorted(os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(GOLDEN, "*.json")))
KEYS = [k for k in FIXTURES if "p" in load_fixture(k) and "n" in load_fixture(k)]


def _build():
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("sha256.hpp", "proofs.hpp", "fpmont.hpp", "codec.hpp", "consts.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-rdynamic", "-std=c++17", "-fPIC", "-shared", "-I" + _EMU, "-I" + _CSRC,
                               "-include", os.path.join(_EMU, "agpr.hpp"), "-include", os.path.join(_EMU, "gmem.hpp"),
                               "-include", os.path.join(_EMU, "imad.hpp"), _SRC, "-o", _SO])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def lib():
    return _build()


# ---- sha256_wire ---------------------------------------------------------------------------------------------------
def _digest(lib, a: bytes, b: bytes, oa: int, ob: int) -> bytes:
    """sha256_wire on copies of a and b that start oa resp. ob bytes into 16-byte aligned buffers."""
    n = len(a)
    bufa = C.create_string_buffer(n + 32)
    bufb = C.create_string_buffer(n + 32)
    base_a = (C.addressof(bufa) + 15) // 16 * 16 + oa
    base_b = (C.addressof(bufb) + 15) // 16 * 16 + ob
    C.memmove(base_a, a, n)
    C.memmove(base_b, b, n)
    out = C.create_string_buffer(32)
    lib.proofs_sha256_wire(C.c_void_p(base_a), C.c_void_p(base_b), C.c_size_t(n), out)
    return out.raw


def test_sha256_wire_matches_hashlib_at_every_length_and_alignment(lib):
    """Every len_each of 0..160 (all residues of the padding position, messages of one to six blocks), the 2L of
    every fixture key and of L = 29, 30, 31 (4L mod 64 = 52: padding fits the last block; 56, 60: it spills into an
    extra one), each with both operands at start offsets 0..3."""
    lens = set(range(161))
    lens |= {2 * load_fixture(k)["fp_bytes"] for k in KEYS}
    lens |= {58, 60, 62}
    assert {(2 * n) % 64 for n in (58, 60, 62)} == {52, 56, 60}
    rng = random.Random(20)
    for n in sorted(lens):
        a, b = rng.randbytes(n), rng.randbytes(n)
        want = hashlib.sha256(a + b).digest()
        for oa in range(4):
            for ob in range(4):
                assert _digest(lib, a, b, oa, ob) == want, (n, oa, ob)


def test_sha256_wire_known_answers(lib):
    """FIPS 180-4 examples that fit the two-operand shape: the empty message, and "abc..." of 56 bytes = 28 || 28."""
    assert _digest(lib, b"", b"", 0, 0).hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    m = b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"
    assert _digest(lib, m[:28], m[28:], 1, 3).hex() == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"


# ---- the response modulo n -------------------------------------------------------------------------------------------
class Order:
    """The parameter block of a key's group order n, as engine.cpp builds it (build_params(n, nl))."""

    def __init__(self, name):
        fx = load_fixture(name)
        self.n, p = int(fx["n"], 16), int(fx["p"], 16)
        self.nl = nl = emu.nl_for(p)
        self.n_len = (self.n.bit_length() + 7) // 8
        R = 1 << (emu.LIMB * nl)
        img = emu.limbs(self.n, nl) + emu.limbs(R % self.n, nl) + emu.limbs(R * R % self.n, nl)
        for K in range(1, emu.KP_MAX + 1):
            img += emu.limbs(K * self.n, nl)
        img += [(-pow(self.n, -1, 1 << emu.LIMB)) % (1 << emu.LIMB), 0, 0, 0]
        self.params = (C.c_uint32 * len(img))(*img)

    def response(self, lib, v, z, a, c, k, lens=None):
        """dl for integer operands; lens = (v_len, z_len, a_len, k_len), default n_len each."""
        ln = lens or (self.n_len,) * 4
        out = C.create_string_buffer(self.n_len)
        rc = lib.proofs_response(self.nl, self.params, self.n_len, v.to_bytes(ln[0], "big"), ln[0], z.to_bytes(ln[1], "big"),
                                 ln[1], a.to_bytes(ln[2], "big"), ln[2], c.to_bytes(32, "big"), k.to_bytes(ln[3], "big"),
                                 ln[3], out)
        assert rc == 0
        return int.from_bytes(out.raw, "big")


@pytest.mark.parametrize("name,nl", [("toy64", 3), ("k256", 10), ("k512", 19), ("k1024", 36), ("k1024b", 37)])
def test_response_matches_python_integers(lib, name, nl):
    """dl = (nonce1 + c * (v + K*z)) mod n, canonical, for operands that need not be reduced: 0, 1, n - 1, n, the
    largest value of n_len bytes, a value whose whole limbs are all ones, a lone top bit — in every combination for
    (v, z, nonce1), with K and c at their extremes (K = 0, c = 2^256 - 1 among them) — and 200 random cases, some
    with shorter operand strings."""
    O = Order(name)
    assert O.nl == nl
    n, top = O.n, 8 * O.n_len
    edges = [0, 1, n - 1, n, (1 << top) - 1, (1 << (emu.LIMB * (top // emu.LIMB))) - 1, 1 << (top - 1)]
    assert all(e < (1 << top) for e in edges)
    rng = random.Random(nl)
    want = lambda v, z, a, c, k: (a + c * (v + k * z)) % n
    cmax = (1 << 256) - 1
    for k in (0, n - 1, (1 << top) - 1, rng.randrange(n)):
        for c in (0, cmax, rng.getrandbits(256)):
            for v in edges:
                for z in edges:
                    for a in edges:
                        assert O.response(lib, v, z, a, c, k) == want(v, z, a, c, k), (v, z, a, c, k)
    for i in range(200):
        lens = tuple(rng.randint(1, O.n_len) if i % 4 == 3 else O.n_len for _ in range(4))
        v, z, a, k = (rng.getrandbits(8 * ln) for ln in lens)
        c = rng.getrandbits(256)
        assert O.response(lib, v, z, a, c, k, lens) == want(v, z, a, c, k), (v, z, a, c, k, lens)
        assert O.response(lib, v, z, a, cmax, 0, lens) == want(v, z, a, cmax, 0)
