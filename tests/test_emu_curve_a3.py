"""CPU: Mult's Miller loop on the isomorphic curve y^2 = x^3 - 3x (option miller_a3; pairing.hpp miller_double with
PairOperands::a3 set, the decode factors of k_decode, the key constant of hostbig.hpp curve_a3_root), on the host
emulation of the device headers with the range checks on: same bytes as the loop on y^2 = x^3 + x and as the golden
vectors, for the windowed loop and the plain NAF."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_fixture

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import emu  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(ROOT, "bgn_amd", "csrc")
_SRC = os.path.join(_HERE, "emu_curve_a3.cpp")
_SO = os.path.join(_EMU, "_build", "libbgn_emu_a3.so")


def _build():
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("fpmont.hpp", "pairing.hpp", "ops.hpp", "codec.hpp", "consts.hpp",
                                                       "fpinv.hpp", "imad.hpp", "hostbig.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-rdynamic", "-std=c++17", "-fPIC", "-shared", "-I" + _EMU, "-I" + _CSRC,
                               "-include", os.path.join(_EMU, "agpr.hpp"), "-include", os.path.join(_EMU, "gmem.hpp"),
                               "-include", os.path.join(_EMU, "imad.hpp"), _SRC, "-o", _SO])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def lib():
    return _build()


def host_root(lib, p):
    """hostbig.hpp curve_a3_root: u with u^4 = -3 mod p, or None."""
    n = (p.bit_length() + 7) // 8
    out = C.create_string_buffer(n)
    ok = lib.a3_root(p.to_bytes(n, "big"), C.c_size_t(n), out)
    return int.from_bytes(out.raw, "big") if ok else None


class Curve:
    """One key on the emulation: decode through the isomorphism, pairing with the switch."""

    def __init__(self, lib, name):
        self.fx = load_fixture(name)
        self.E = emu.Emu.from_fixture(self.fx)
        self.lib, self.p, self.nl = lib, self.E.p, self.E.nl
        self.u = host_root(lib, self.p)
        R2 = pow(1 << (emu.LIMB * self.nl), 2, self.p)
        arr = lambda v: (C.c_uint32 * self.nl)(*emu.limbs(v, self.nl))
        self.factors = (arr(self.u ** 2 * R2 % self.p), arr(self.u ** 3 * R2 % self.p)) if self.u else None
        self.cts = [bytes.fromhex(e["ct"]) for e in self.fx["encrypt"]]

    def decode(self, wire, a3):
        out = (C.c_uint32 * (2 * self.nl))()
        f = self.factors if a3 else (None, None)
        assert self.lib.a3_decode(self.nl, self.E.params, wire, self.E.L, f[0], f[1], out) == 0
        return out

    def pairing(self, a, b, a3, windowed):
        out = (C.c_uint32 * (2 * self.nl))()
        assert self.lib.a3_pairing(self.nl, self.E.params, self.E.consts, self.decode(a, a3), self.decode(b, a3),
                                   1 if a3 else 0, 1 if windowed else 0, out) == 0
        return self.E.encode(out)


@pytest.mark.parametrize("name", ["toy64", "k256", "k512", "k1024", "k1024b"])
def test_host_constant_is_a_fourth_root_of_minus_three(lib, name):
    """For every fixture key with p = 1 mod 3 the host finds u with u^4 = -3; for the others (k1024b) the route is off."""
    p = int(load_fixture(name)["p"], 16)
    u = host_root(lib, p)
    if p % 3 == 1:
        assert u is not None and 0 < u < p and pow(u, 4, p) == p - 3
    else:
        assert u is None
    assert (p % 3 == 1) == (name != "k1024b") or name == "toy64"      # the bench key and the small keys admit it


@pytest.mark.parametrize("name,rows", [("k256", 3), ("k512", 2), ("k1024", 1)])
def test_a3_pairing_gives_the_golden_bytes(lib, name, rows):
    """The golden Mult inputs through the decode factors and the a = -3 doubling step, range checks on: the bytes of the
    a = 1 path and of the fixture, for the width-5 loop and the plain NAF.  The decoded operands really are the images
    (u^2 x, u^3 y) in Montgomery form."""
    K = Curve(lib, name)
    assert K.u is not None and pow(K.u, 4, K.p) == K.p - 3
    fx, cts = K.fx, K.cts
    K.E.set_window(5)
    R = 1 << (emu.LIMB * K.nl)
    a0 = cts[fx["mult"][0]["a"]]
    x, y = int.from_bytes(a0[:K.E.L], "big"), int.from_bytes(a0[K.E.L:], "big")
    m = K.decode(a0, True)
    val = lambda k: sum(int(m[k * K.nl + j]) << (emu.LIMB * j) for j in range(K.nl))
    assert val(0) == K.u ** 2 * x * R % K.p and val(1) == K.u ** 3 * y * R % K.p
    picked = [v for v in fx["mult"] if any(cts[v["a"]]) and any(cts[v["b"]])][:rows]
    assert len(picked) == rows
    for v in picked:
        a, b = cts[v["a"]], cts[v["b"]]
        for windowed in (True, False):
            got = K.pairing(a, b, True, windowed)
            assert got.hex() == v["out"], (name, windowed)
            assert got == K.pairing(a, b, False, windowed), (name, windowed)


def test_a3_pairing_of_dependent_points(lib):
    """B = A and B = -A (the pairing of linearly dependent points) on the image curve: the bytes of the a = 1 path."""
    K = Curve(lib, "k256")
    L = K.E.L
    a = next(c for c in K.cts if any(c))
    neg = a[:L] + ((K.p - int.from_bytes(a[L:], "big")) % K.p).to_bytes(L, "big")
    for b in (a, neg):
        for windowed in (True, False):
            assert K.pairing(a, b, True, windowed) == K.pairing(a, b, False, windowed)


@pytest.mark.parametrize("name", ["k256", "k512", "k1024"])
def test_a3_step_programs_stay_in_range_on_extreme_residues(lib, name):
    """The step programs with the switch on, from states whose limbs are all ones, alternating, or a lone top limb
    (the residues of test_emu_kernels.py::test_emu_products_at_extreme_limbs), lifted to the documented bounds of the
    state (X < 8p, Y < 2p, Z < 4p, f < 2p): the emulation aborts on a carry out of the top limb, a negative
    difference or an accumulator that would wrap."""
    K = Curve(lib, name)
    p, nl = K.p, K.nl
    ones = (1 << (p.bit_length() - 1)) - 1
    full = (1 << p.bit_length()) - 1 if (1 << p.bit_length()) - 1 < 2 * p else 2 * p - 1
    stripes = sum(emu.MASK << (emu.LIMB * j) for j in range(0, nl, 2))
    lone = 1 << (p.bit_length() - 1)
    pats = [full, ones, ones & stripes, ones & ~stripes, lone, 2 * p - 1, p - 1, 1]
    assert all(0 < v < 2 * p for v in pats)
    arr = lambda vals: (C.c_uint32 * (nl * len(vals)))(*[w for v in vals for w in emu.limbs(v, nl)])
    out = (C.c_uint32 * (5 * nl))()
    for i, v in enumerate(pats):
        w = pats[(i + 3) % len(pats)]
        for lift in (0, 1):                                       # the residues as they are, and at the top of the bounds
            state = [v + 6 * p * lift, w, v + 2 * p * lift, w, v]
            assert state[0] < 8 * p and state[2] < 4 * p
            ops_a, ops_b = arr([w % p, v % p]), arr([v % p, w % p])
            assert lib.a3_steps(nl, K.E.params, arr(state), ops_a, ops_b, 1, out) == 0
            assert all(int(x) <= emu.MASK for x in out)
