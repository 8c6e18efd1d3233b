"""CPU: the lane-level models of the two split-limb kernel families (tests/coop_model.py LaneMachine, tests/quad_model.py
QuadLaneMachine) on the extreme operands of tests/extreme_operands.py, composed as the diagnostic kernels compose the
families' routines (kern_coop.hip k_field_ops_coop, kern_quad.hip k_field_ops_quad): operands as stored values or as
two-term sums behind one carry pass, Montgomery product, one carry pass, product with the raw 1, canonical limbs.
Compared with Python integers at every limb count a fixture key has.  tests/test_gpu_family_field.py runs the compiled
kernels on the same list: a disagreement there is then either "the model is wrong too" or "the compiled code differs".

Sub-sample (the numpy models take milliseconds per product): EVERY pair of the operand list (special x special), every
targeted pair, and the first N_RANDOM_HERE random pairs; the squares are computed once per distinct operand."""
import numpy as np
import pytest

import coop_model as cm
import quad_model as qm
from conftest import load_fixture
from extreme_operands import LIMB_BITS, N_RANDOM, OUTPUTS, expected, limbs_for, operands, pairs

I64 = np.int64
I32 = np.int32
N_RANDOM_HERE = 8


def _sample(p, nl):
    ps, nsq = pairs(p, nl)
    return ps[:len(ps) - N_RANDOM + N_RANDOM_HERE], nsq


class CoopField:
    """k_field_ops_coop on the lane machine."""

    def __init__(self, p, nl):
        self.m = cm.LaneMachine(p, nl)
        self.nl = nl
        self.raw1 = cm.to_lanes(1, nl)
        self.p_l = self.m.p_l.astype(I64)

    def load(self, v):
        return cm.to_lanes(self.m.mont(v), self.nl)

    def combo(self, x, y, cy, k):                                  # coop_combo / the sums of coop_operand: 1*x + cy*y + k*p
        return x.astype(I32).astype(I64) + I64(cy) * y.astype(I32).astype(I64) + I64(k) * self.p_l

    def norm(self, acc):
        return self.m.normalize64(acc)

    def product(self, a, b):
        return self.norm(self.m.mul(a, b))

    def leave(self, t):
        r = self.m.canonical(self.product(t, self.raw1))
        assert np.all(r >= 0) and np.all(r <= cm.MASK)
        return cm.from_lanes(r.astype(np.int64).astype(np.uint32))


class QuadField:
    """k_field_ops_quad on the lane machine."""

    def __init__(self, p, nl):
        self.m = qm.QuadLaneMachine(p, nl)
        self.nl = nl
        self.raw1 = qm.to_quad(1, nl)
        self.p_l = self.m.p_q

    def load(self, v):
        return qm.to_quad(self.m.mont(v), self.nl)

    def combo(self, x, y, cy, k):                                  # quad_combo: 1*x + cy*y + k*p
        return x.astype(I64) + I64(cy) * y.astype(I64) + I64(k) * self.p_l

    def norm(self, acc):
        return self.m.normalize(acc)

    def product(self, a, b):
        return self.norm(self.m.mul(a, b))

    def leave(self, t):
        return qm.from_quad(self.m.canonical(self.product(t, self.raw1)))


def _run(F, tag, p, nl):
    f = F(p, nl)
    ps, nsq = _sample(p, nl)
    assert nsq == len(operands(p, nl)) ** 2 and ps[nsq - 1] == (operands(p, nl)[-1],) * 2 and len(ps) > nsq
    squares = {}
    for i, (x, y) in enumerate(ps):
        a, b = f.load(x), f.load(y)
        for v, l in ((x, a), (y, b)):
            if v not in squares:
                squares[v] = f.leave(f.product(l, l))
        got = (f.leave(f.product(a, b)),
               f.leave(f.product(f.norm(f.combo(a, b, -1, 1)), f.norm(f.combo(a, b, 1, 0)))),
               squares[x], squares[y],
               f.leave(f.norm(f.combo(a, b, 1, 0))),
               f.leave(f.norm(f.combo(a, b, -1, 1))))
        want = expected(p, x, y)
        for k, name in enumerate(OUTPUTS):
            assert got[k] == want[k], "%s model, %d limbs: element %d (x = %#x, y = %#x), output %s: got %#x, want %#x" % (
                tag, nl, i, x, y, name, got[k], want[k])


@pytest.mark.parametrize("name", ["toy64", "k256", "k512", "k1024", "k1024b"])
def test_cooperative_lane_model_on_extreme_operands(name):
    p = int(load_fixture(name)["p"], 16)
    nl = limbs_for(p)
    assert nl == cm.nl_for(p) and LIMB_BITS == cm.LIMB
    _run(CoopField, "cooperative", p, nl)


@pytest.mark.parametrize("name", ["k256", "k512", "k1024", "k1024b", "k2048"])
def test_lane_group_model_on_extreme_operands(name):
    p = int(load_fixture(name)["p"], 16)
    nl = limbs_for(p)
    assert nl == qm.nl_for(p)
    _run(QuadField, "lane-group", p, nl)
