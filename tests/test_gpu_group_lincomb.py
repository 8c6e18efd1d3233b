"""GPU: the column-group path of bgn_lincomb_batch / _dev for narrow weights (csrc/groupops.hpp) — the same map, the
same bytes.

The expected bytes are those of test_gpu_lincomb.py: the C oracle's encryption of sums taken in Python integers over
ciphertexts of known exponents, never the table path's output.  Every case runs with the group size forced to 5, 2 and 6
and the chunks to 1 and 3 (cut on group boundaries), and once more on the table path.  problem() spreads its equal,
opposite and identity ciphertexts over the vector; the degenerate case puts them into ONE group — (A, A, -A, identity, B)
— under every trit pattern, so the table build meets a doubling, an identity entry and an identity operand."""
import itertools
import random

import numpy as np
import pytest

from conftest import engine_key
from test_gpu_lincomb import problem
from test_gpu_sum import ALL_KEYS, material

pytestmark = pytest.mark.gpu

SHAPES = {(1, 1, 1): 1, (1, 65, 4): 1, (2, 3, 6): 2, (1, 65, 33): 4}      # (nvec, nrows, d): w_bits
CASES = [(k, s) for k in ALL_KEYS for s in SHAPES if not (k == "k2048" and s == (1, 65, 33))]
SETTINGS = [{"lin_groups": 5}, {"lin_groups": 2}, {"lin_groups": 6}, {"lin_groups": 5, "lin_split": 1}, {"lin_groups": 5, "lin_split": 3}]
WALK = {1: "k_grp_walk_g1", 2: "k_grp_walk_gt"}
TABLE = {1: "k_grp_table_g1", 2: "k_grp_table_gt"}


def run_every_setting(eng, engopts, level, ct, W, wb, nvec, want):
    for setting in SETTINGS:
        for opt, k in setting.items():
            engopts.set(opt, k)
        got = eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes()
        assert eng.last_kernel_name() == WALK[level] and eng.last_aux_kernel_name() == TABLE[level], setting
        assert got == want, setting
        for opt in setting:
            engopts.unset(opt)
    engopts.set("lin_groups", 0)
    assert eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes() == want, "tables"
    assert eng.last_kernel_name() == ("k_lin_walk_g1" if level == 1 else "k_lin_walk_gt")


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name,shape", CASES, ids=["%s-%dx%dx%d" % ((k,) + s) for k, s in CASES])
def test_the_group_path_gives_the_oracles_bytes_under_every_setting(name, shape, level, engopts):
    m = material(name)
    eng = engine_key(m.fx)[0].engine
    nvec, nrows, d = shape
    wb = SHAPES[shape]
    _, W, ct, want, _ = problem(m, level, nvec, nrows, d, wb, "grp-%s-%d-%s" % (name, level, shape))
    run_every_setting(eng, engopts, level, ct, W, wb, nvec, want)


@pytest.mark.parametrize("level", [1, 2])
def test_equal_opposite_and_identity_ciphertexts_in_one_group(level, engopts):
    m = material("k256")
    eng = engine_key(m.fx)[0].engine
    n = m.n
    # pool entries: level 1 (1, 0), (1, 0), (n-1, 0), the identity, a random pair; level 2 g, g, g^-1, 1, g^2
    idx = np.array([[1, 1, 3, 0, 5 if level == 1 else 2]])
    rows = list(itertools.product((-1, 0, 1), repeat=5)) + [(3, -2, 1, 0, -3)]      # w_bits = 1: counts as (1, 0, 1, 0, -1)
    W = np.array(rows, dtype=np.int32)
    assert not W[121].any()                                                        # the all-zero row
    eff = np.sign(W) * (np.abs(W) % 2)
    exps = m.exp1 if level == 1 else [(e,) for e in m.exp2]
    totals = [tuple(sum(int(eff[r, j]) * exps[idx[0, j]][c] for j in range(5)) % n for c in range(len(exps[0])))
              for r in range(len(rows))]
    want = m.expect(level, totals if level == 1 else [t[0] for t in totals])
    run_every_setting(eng, engopts, level, m.wire(level, idx), W, 1, 1, want)


def test_blinded_group_maps(engopts):
    """One r per result, as test_gpu_lincomb.test_blinded_linear_maps."""
    m = material("k1024b")
    eng = engine_key(m.fx)[0].engine
    o, n = m.o, m.n
    rng = random.Random("grp-blind")
    engopts.set("lin_groups", 5)
    for level in (1, 2):
        _, W, ct, want, totals = problem(m, level, 2, 3, 7, 2, "grp-blind-%d" % level)
        rs = [0] + [rng.randrange(n) for _ in range(5)]
        got = eng.lincomb(level, ct, W, w_bits=2, r=rs, nvec=2).tobytes()
        assert eng.last_kernel_name() == WALK[level]
        if level == 1:
            want = o.encrypt([t[0] for t in totals], [(t[1] + r) % n for t, r in zip(totals, rs)])
        else:
            if m.eqq is None:
                Q = bytes.fromhex(m.fx["Q"])
                m.eqq = o.mult(Q, Q)
            want = o.add(2, want, o.multconst(2, m.eqq * 6, rs))
        assert got == want, level


@pytest.mark.parametrize("level", [1, 2])
def test_device_arrays_at_odd_byte_addresses_with_guard_bytes(level, engopts):
    import torch
    m = material("k256")
    eng = engine_key(m.fx)[0].engine
    nvec, nrows, d, G = 2, 3, 7, 64
    _, W, ct, want, _ = problem(m, level, nvec, nrows, d, 2, "grp-dev-%d" % level)
    ct = np.frombuffer(ct, dtype=np.uint8)
    d_w = torch.from_numpy(W.copy()).cuda()
    engopts.set("lin_groups", 5)
    for off_in, off_out in [(1, 3), (2, 1), (3, 2)]:
        d_in = torch.zeros(len(ct) + 8, dtype=torch.uint8, device="cuda")
        d_in[off_in:off_in + len(ct)] = torch.from_numpy(ct.copy()).cuda()
        d_out = torch.full((2 * G + len(want) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = G + off_out
        eng.lincomb_dev(level, d_in[off_in:], d_w, 2, d_out[lo:], nvec, nrows, d)
        torch.cuda.synchronize()
        assert eng.last_kernel_name() == WALK[level]
        h = d_out.cpu().numpy()
        assert h[lo:lo + len(want)].tobytes() == want, (off_in, off_out)
        assert (h[:lo] == 0xA5).all() and (h[lo + len(want):] == 0xA5).all(), (off_in, off_out)
