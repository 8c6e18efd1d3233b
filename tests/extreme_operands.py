"""Operands that stress the carry chains of the split-limb kernel families (bgn_amd/csrc/coop/coop.hpp: one 29-bit
limb per lane; bgn_amd/csrc/quad/quad.hpp: M = ceil(NL / 4) limbs in each of four lanes), and what the diagnostic
entry point bgn_field_ops_family_batch must answer for them, on Python integers.  One list for the GPU test
(tests/test_gpu_family_field.py) and for the CPU test of the lane-level models (tests/test_family_models_extreme.py):
kernel, model and integers are pinned to the same operands.
TEST INFRASTRUCTURE: not used by the product.
"""
from __future__ import annotations

import random

from bgn_amd.synthetic import LIMB_BITS, limbs_for

N_RANDOM = 256
FAMILY_LIMBS = {1: (3, 10, 19, 36, 37), 2: (10, 19, 36, 37, 72)}     # kern_coop.hip / kern_quad.hip: the instantiations
FAMILY_NAMES = {1: "cooperative", 2: "lane groups"}
OUTPUTS = ("x*y", "(x-y)*(x+y)", "x^2", "y^2", "x+y", "x-y")


def _unique(vs):
    out = []
    for v in vs:
        if v not in out:
            out.append(v)
    return out


def montgomery_extremes(p: int, nl: int):
    """Integers whose limbs are extreme — every limb below the top one all ones, alternating full and empty limbs, the
    same shifted by a limb, a lone top limb, full minus alternating — as tests/test_gpu_holes.py builds them for the
    lane kernels.  As Montgomery residues they are what the rows of a product multiply."""
    low = LIMB_BITS * ((p.bit_length() - 1) // LIMB_BITS)
    full = ((p >> low) - 1 << low) | ((1 << low) - 1) if (p >> low) > 1 else (1 << low) - 1
    alt = sum(((1 << LIMB_BITS) - 1) << (LIMB_BITS * j) for j in range(0, low // LIMB_BITS, 2))
    res = [full, alt, (alt << LIMB_BITS) % (1 << low), (p >> low) << low, full - alt]
    assert all(0 <= v < p for v in res)
    return res


def operands(p: int, nl: int):
    """The list of single operands (plain residues below p, no duplicates)."""
    m = (nl + 3) // 4
    r_inv = pow(1 << (LIMB_BITS * nl), -1, p)
    special = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << (p.bit_length() - 1)]
    boundary = []
    for j in (1, m, 2 * m, 3 * m, nl - 1):                      # a limb, the three lane boundaries, the top limb
        boundary += [((1 << (LIMB_BITS * j)) - 1) % p, (1 << (LIMB_BITS * j)) % p]
    mont = [v * r_inv % p for v in montgomery_extremes(p, nl)]  # the product's rows see the extreme limbs themselves
    out = _unique(special + boundary + mont)
    assert all(0 <= v < p for v in out)
    return out


def targeted_pairs(p: int, nl: int):
    """Pairs whose results sit at the ends of the canonical step's carry and borrow chains."""
    m = (nl + 3) // 4
    r_inv = pow(1 << (LIMB_BITS * nl), -1, p)
    full = montgomery_extremes(p, nl)[0]
    targets = _unique([0, 1, p - 1, ((1 << (LIMB_BITS * m)) - 1) % p, full * r_inv % p])
    out = []
    for x in operands(p, nl):
        if x:
            out += [(x, t * pow(x, -1, p) % p) for t in targets]     # x*y = t exactly
            out.append((x, p - x))                                   # x + y = p exactly
        out.append((x, p - 1 - x))                                   # x + y = p - 1
        out.append((x, x))                                           # x - y = 0
    return out


def pairs(p: int, nl: int, seed: int = 20240917):
    """(all pairs of operands(), the targeted pairs, N_RANDOM seeded random pairs) as one list, with the number of
    special x special pairs in front."""
    ops = operands(p, nl)
    sq = [(x, y) for x in ops for y in ops]
    rng = random.Random(seed)
    rnd = [(rng.randrange(p), rng.randrange(p)) for _ in range(N_RANDOM)]
    out = sq + targeted_pairs(p, nl) + rnd
    assert all(0 <= x < p and 0 <= y < p for x, y in out), "an operand is not below p"
    return out, len(sq)


def expected(p: int, x: int, y: int):
    """The six outputs in the order of OUTPUTS: prod = [0] || [1], sqr = [2] || [3], lin = [4] || [5]."""
    return (x * y % p, (x - y) * (x + y) % p, x * x % p, y * y % p, (x + y) % p, (x - y) % p)


def wire(ps, L: int) -> bytes:
    return b"".join(x.to_bytes(L, "big") + y.to_bytes(L, "big") for x, y in ps)


def compare(tag, p: int, L: int, ps, prod, sqr, lin):
    """Byte-exact comparison of the three output arrays (count x 2L bytes) with Python integers; the assertion names
    (tag..., index, output)."""
    bufs = (bytes(prod), bytes(sqr), bytes(lin))
    assert all(len(b) == 2 * L * len(ps) for b in bufs), (tag, [len(b) for b in bufs])
    for i, (x, y) in enumerate(ps):
        want = expected(p, x, y)
        for k, name in enumerate(OUTPUTS):
            off = i * 2 * L + (k & 1) * L
            got = bufs[k >> 1][off:off + L]
            assert got == want[k].to_bytes(L, "big"), "%s: element %d (x = %#x, y = %#x), output %s: got %#x, want %#x" % (
                tag, i, x, y, name, int.from_bytes(got, "big"), want[k])
