"""GPU: the multi-precision arithmetic of the two split-limb kernel families on its own (bgn_field_ops_family_batch:
family 1 = the wave-cooperative kernels, coop/coop.hpp, one 29-bit limb per lane; family 2 = the lane groups,
quad/quad.hpp, M = ceil(NL / 4) limbs in each of four lanes) against Python integers, byte for byte, on operands whose
plain and Montgomery limbs are extreme (tests/extreme_operands.py) — what the coordinates of valid random points, all
these routines otherwise see on the GPU, reach with probability 2^-29 per limb: carries that ripple across a lane
boundary, values that canonicalise from exactly p or p - 1, all-ones rows of a product.  The lane-level models run the
same list on the CPU (tests/test_family_models_extreme.py).

(family, limbs) that run: cooperative at 3, 10, 19, 36, 37; lane groups at 10 (top limb at index 0 of lane 3), 19, 36,
37 (index 6 of 10) and 72 (18 limbs per lane: the mid-life carry of an accumulator).  Elements per case: every pair of
the operand list (19 to 23 operands), the targeted pairs and 256 random pairs — 763 at 3 limbs, 859 at 10 and 19,
963 from 36 limbs on.

Then, through the public route and no diagnostic code: level-2 MultConst of bases taken from the same list, forced
onto the lane groups and onto the one-element-per-lane kernel, against square-and-multiply on Python integers."""
import pytest

from conftest import engine_key, load_fixture
from extreme_operands import FAMILY_LIMBS, FAMILY_NAMES, N_RANDOM, compare, limbs_for, operands, pairs, targeted_pairs, wire
from test_gpu_multconst_l2 import fp2_pow

pytestmark = pytest.mark.gpu

COOP, QUAD = 1, 2
CASES = [(COOP, k) for k in ("toy64", "k256", "k512", "k1024", "k1024b")] + \
        [(QUAD, k) for k in ("k256", "k512", "k1024", "k1024b", "k2048")]


def _setup(family, name):
    fx = load_fixture(name)
    pk, _ = engine_key(fx)
    p = int(fx["p"], 16)
    nl = limbs_for(p)
    assert nl in FAMILY_LIMBS[family]
    return pk.engine, p, nl, "%s, %s (%d limbs)" % (FAMILY_NAMES[family], name, nl)


@pytest.mark.parametrize("family,name", CASES)
def test_family_field_arithmetic_on_extreme_operands_vs_python_integers(family, name):
    eng, p, nl, tag = _setup(family, name)
    L = eng.L
    ps, nsq = pairs(p, nl)
    assert nsq == len(operands(p, nl)) ** 2 >= 19 * 19 and len(ps) == nsq + len(targeted_pairs(p, nl)) + N_RANDOM
    assert all(0 <= x < p and 0 <= y < p for x, y in ps)
    prod, sqr, lin = eng.field_ops_family(family, wire(ps, L))
    compare(tag, p, L, ps, prod.tobytes(), sqr.tobytes(), lin.tobytes())


@pytest.mark.parametrize("family,name", CASES)
def test_family_field_arithmetic_at_ragged_counts(family, name):
    """One element; counts that are no multiple of the elements per workgroup (4 waves / 64 quads) or per wave (16
    quads); the elements come from both ends of the list, so that the stand-ins of a ragged tail differ from their
    neighbours."""
    eng, p, nl, tag = _setup(family, name)
    L = eng.L
    ps, nsq = pairs(p, nl)
    for count in (1, 3, 67, 129):
        sub = ps[-(count // 2 + 1):] + ps[nsq - 5:nsq - 5 + count // 2]
        assert len(sub) == count
        prod, sqr, lin = eng.field_ops_family(family, wire(sub, L))
        compare("%s, count %d" % (tag, count), p, L, sub, prod.tobytes(), sqr.tobytes(), lin.tobytes())
    prod, sqr, lin = eng.field_ops_family(family, b"")
    assert prod.shape == sqr.shape == lin.shape == (0, 2 * L)


@pytest.mark.parametrize("family,name", [(COOP, "k2048"), (QUAD, "toy64"), (3, "k256"), (0, "k256")])
def test_a_family_without_an_instantiation_is_an_argument_error(family, name):
    """72 limbs do not fit the 64 lanes of a wave; 3 limbs are fewer than two per lane; there are two families."""
    import bgn_amd
    from bgn_amd._lib import BGN_E_ARG
    fx = load_fixture(name)
    pk, _ = engine_key(fx)
    eng = pk.engine
    with pytest.raises(bgn_amd.BgnError) as ei:
        eng.field_ops_family(family, bytes(2 * eng.L))
    assert ei.value.code == BGN_E_ARG
    assert ("no instantiation" in str(ei.value)) == (family in (COOP, QUAD)), str(ei.value)
    # ... and the context works afterwards
    prod, _, _ = eng.field_ops_family(QUAD if name != "toy64" else COOP, (3).to_bytes(eng.L, "big") + (5).to_bytes(eng.L, "big"))
    assert int.from_bytes(prod.tobytes()[:eng.L], "big") == 15


# ---------------------------------------------------------------- level-2 MultConst on bases with extreme limbs
@pytest.mark.parametrize("name", ["k256", "k1024", "k1024b", "k2048"])
def test_multconst_l2_of_extreme_bases_on_the_lane_groups_and_the_lane_kernel(name, engopts):
    """base^k in F_p^2 for bases (re, im) from the operand list — none of them a ciphertext — and k in {0, 1, 2, 3, 15,
    16, 17, n - 1, n + 1} (the window digits of the lane groups' power around a digit boundary): every third pair of the
    list, about 180 elements, the exponents in turn."""
    fx = load_fixture(name)
    pk, _ = engine_key(fx)
    eng = pk.engine
    p, n = int(fx["p"], 16), int(fx["n"], 16)
    L = eng.L
    ops = operands(p, limbs_for(p))
    bases = [(x, y) for x in ops for y in ops][::3]
    assert 120 <= len(bases) <= 240
    kset = [0, 1, 2, 3, 15, 16, 17, n - 1, n + 1]
    ks = [kset[i % len(kset)] for i in range(len(bases))]
    want = [fp2_pow(b, k, p) for b, k in zip(bases, ks)]
    buf = wire(bases, L)
    for kernel in ("quad", "lane"):
        engopts.set("quad_max_mc", (1 << 40) if kernel == "quad" else 0)
        got = eng.multconst(2, buf, ks).tobytes()
        assert ("quad" in eng.last_kernel_name()) == (kernel == "quad"), eng.last_kernel_name()
        for i, (b, k, w) in enumerate(zip(bases, ks, want)):
            row = got[i * 2 * L:(i + 1) * 2 * L]
            g = (int.from_bytes(row[:L], "big"), int.from_bytes(row[L:], "big"))
            assert g == w, "%s, %s kernel: element %d, base (%#x, %#x), k = %#x: got (%#x, %#x), want (%#x, %#x)" % (
                name, kernel, i, b[0], b[1], k, g[0], g[1], w[0], w[1])
