"""CPU: one reduction pass of the segmented sums (csrc/sumops.hpp) on the host emulation of the device headers, against
Python integers: which elements lane (s, t) of a pass walks (t, t + split, ...: sum_lane / sum_run_len), and the lane
functions that accumulate them — level 1 by the Jacobian accumulator against a plain affine group law on
y^2 = x^3 + x, level 2 by the Barrett product and by the Montgomery accumulator against (a + bi)(c + di) mod p.  The
elements come from a small pool (the identity, a point, its double, their negatives; 1, h, h^2, 1/h), so identities,
equal points and opposite points meet the accumulators at many positions; one segment is all identities and one sums to
the identity.  Splits 1, 7 and 64 over lengths 1, 2, 63, 65 and 257, and one split wider than a workgroup."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, load_fixture

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import emu  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(ROOT, "bgn_amd", "csrc")
_SRC = os.path.join(_HERE, "emu_sum.cpp")
_SO = os.path.join(_EMU, "_build", "libbgn_emu_sum.so")

KEYS = ["toy64", "k256", "k512", "k1024", "k1024b"]          # 3, 10, 19, 36 and 37 limbs
LENS = (1, 2, 63, 65, 257)
SPLITS = (1, 7, 64)


def _build():
    os.makedirs(os.path.dirname(_SO), exist_ok=True)
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("sumops.hpp", "ops.hpp", "barrett.hpp", "fpmont.hpp", "fpinv.hpp",
                                                      "codec.hpp", "consts.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-rdynamic", "-std=c++17", "-fPIC", "-shared", "-I" + _EMU, "-I" + _CSRC,
                               "-include", os.path.join(_EMU, "agpr.hpp"), "-include", os.path.join(_EMU, "gmem.hpp"),
                               "-include", os.path.join(_EMU, "imad.hpp"), _SRC, "-o", _SO])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def lib():
    return _build()


# ---- the reference: Python integers -----------------------------------------------------------------------------------
def g1_add(A, B, p):
    """Affine addition on y^2 = x^3 + x; None is the identity."""
    if A is None:
        return B
    if B is None:
        return A
    (x1, y1), (x2, y2) = A, B
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + 1) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def gt_mul(A, B, p):
    return (A[0] * B[0] - A[1] * B[1]) % p, (A[0] * B[1] + A[1] * B[0]) % p


class Key:
    def __init__(self, name):
        fx = load_fixture(name)
        self.p = p = int(fx["p"], 16)
        self.nl = nl = emu.nl_for(p)
        self.L = L = fx["fp_bytes"]
        R = 1 << (emu.LIMB * nl)
        img = emu.limbs(p, nl) + emu.limbs(R % p, nl) + emu.limbs(R * R % p, nl)
        for K in range(1, emu.KP_MAX + 1):
            img += emu.limbs(K * p, nl)
        img += [(-pow(p, -1, 1 << emu.LIMB)) % (1 << emu.LIMB), 0, 0, 0]
        self.params = (C.c_uint32 * len(img))(*img)
        self.mu = (C.c_uint32 * (nl + 2))(*emu.limbs((1 << (2 * emu.LIMB * nl)) // p, nl + 2))
        Pw = bytes.fromhex(fx["P"])
        G = (int.from_bytes(Pw[:L], "big"), int.from_bytes(Pw[L:], "big"))
        assert (G[1] * G[1] - G[0] ** 3 - G[0]) % p == 0
        G2 = g1_add(G, G, p)
        rng = random.Random("emu-sum-" + name)
        more = []
        for _ in range(4):                                # a few other multiples of the generator
            k, acc, base = rng.randrange(3, 1 << 40), None, G
            while k:
                if k & 1:
                    acc = g1_add(acc, base, p)
                base = g1_add(base, base, p)
                k >>= 1
            more.append(acc)
        neg = lambda A: (A[0], (p - A[1]) % p)
        self.pool1 = [None, G, G2, neg(G), neg(G2)] + more
        hw = bytes.fromhex(fx["mult"][0]["out"])          # a GT element of the fixture
        h = (int.from_bytes(hw[:L], "big"), int.from_bytes(hw[L:], "big"))
        assert (h[0] * h[0] + h[1] * h[1]) % p == 1
        self.pool2 = [(1, 0), h, gt_mul(h, h, p), (h[0], (p - h[1]) % p)]

    def wire(self, level, v):
        if v is None:
            return bytes(2 * self.L)
        return v[0].to_bytes(self.L, "big") + v[1].to_bytes(self.L, "big")

    def fold(self, level, vals):
        acc = None if level == 1 else (1, 0)
        for v in vals:
            acc = g1_add(acc, v, self.p) if level == 1 else gt_mul(acc, v, self.p)
        return acc


_KEYS = {}


def key(name):
    if name not in _KEYS:
        _KEYS[name] = Key(name)
    return _KEYS[name]


def content(k, level, nseg, length, seed):
    rng = random.Random(seed)
    pool = k.pool1 if level == 1 else k.pool2
    small = 5 if level == 1 else 4
    rows = [[pool[rng.randrange(len(pool) if s % 2 == 0 else small)] for _ in range(length)] for s in range(nseg)]
    if nseg >= 2:                                         # a segment that sums to the identity
        a, b = (pool[1], pool[3])
        rows[1] = [a if j % 2 == 0 else b for j in range(length - length % 2)] + [pool[0]] * (length % 2)
        assert k.fold(level, rows[1]) == (None if level == 1 else (1, 0))
    if nseg >= 3:                                         # a segment of identities
        rows[2] = [pool[0]] * length
    return rows


def run_pass(lib, k, mode, rows, split):
    level = 1 if mode == 1 else 2
    nseg, length = len(rows), len(rows[0])
    E = 2 * k.L
    src = b"".join(k.wire(level, v) for r in rows for v in r)
    out = C.create_string_buffer(nseg * split * E)
    rc = lib.sum_emu_pass(k.nl, k.params, k.mu, (k.p - 2).bit_length(), mode, src, k.L, C.c_uint64(nseg), length, split, out)
    assert rc == 0, rc
    got = [[out.raw[(s * split + t) * E:(s * split + t + 1) * E] for t in range(split)] for s in range(nseg)]
    want = [[k.wire(level, k.fold(level, r[t::split])) for t in range(split)] for r in rows]
    return got, want


@pytest.mark.parametrize("mode", [1, 2, 3], ids=["g1", "gt-barrett", "gt-montgomery"])
@pytest.mark.parametrize("name", KEYS)
def test_a_pass_equals_python_integers(lib, name, mode):
    k = key(name)
    level = 1 if mode == 1 else 2
    assert lib.sum_emu_block() == 256
    for length in LENS:
        rows = content(k, level, 3, length, "%s-%d-%d" % (name, mode, length))
        for split in SPLITS:
            split = min(split, length)
            got, want = run_pass(lib, k, mode, rows, split)
            assert got == want, (name, mode, length, split)
            if split == 1:
                assert got[2][0] == k.wire(level, None if level == 1 else (1, 0))
                if length > 1:
                    assert got[1][0] == got[2][0]


@pytest.mark.parametrize("mode", [1, 2])
def test_a_split_wider_than_a_workgroup_and_the_passes_behind_it(lib, mode):
    """600 elements in 300 lanes (two workgroups per segment, the second ragged), then 300 -> 7 -> 1: the partials of
    each pass are the next one's elements, and the end is the plain fold."""
    k = key("toy64")
    level = 1 if mode == 1 else 2
    rows = content(k, level, 2, 600, "wide-%d" % mode)
    cur = rows
    for split in (300, 7, 1):
        got, want = run_pass(lib, k, mode, cur, split)
        assert got == want, split
        L = k.L
        dec = lambda w: (None if level == 1 and not any(w) else (int.from_bytes(w[:L], "big"), int.from_bytes(w[L:], "big")))
        cur = [[dec(w) for w in r] for r in got]
    assert [r[0] for r in cur] == [k.fold(level, r) for r in rows]


def test_level_2_reduces_residues_at_or_above_p(lib):
    k = key("k256")
    p, L = k.p, k.L
    top = min(1 << (8 * L), 1 << (emu.LIMB * k.nl))
    rows = [[(p, 1), (p + 1, p), (top - 1, top - 2), (5, 7), (top - 1, 0)]]
    for mode in (2, 3):
        got, _ = run_pass(lib, k, mode, rows, 1)
        acc = (1, 0)
        for v in rows[0]:
            acc = gt_mul(acc, (v[0] % p, v[1] % p), p)
        assert got[0][0] == k.wire(2, acc), mode
        got, _ = run_pass(lib, k, mode, rows, 5)              # a lane with one element copies it, reduced
        assert got[0] == [k.wire(2, (v[0] % p, v[1] % p)) for v in rows[0]], mode
