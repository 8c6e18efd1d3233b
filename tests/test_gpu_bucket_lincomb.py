"""GPU: the bucket path of bgn_lincomb_batch / _dev (csrc/bucketops.hpp) — the same map, the same bytes, no tables.

The expected bytes are those of test_gpu_lincomb.py: the C oracle's encryption of sums taken in Python integers over
ciphertexts of known exponents.  problem() plants what matters inside one bucket — (+k, -k) and (k, k) on two copies of
one ciphertext, an identity ciphertext, an all-zero row, a weight above 2^w_bits; the pattern "equal" makes every weight
of a row the same, so one bucket of a window holds all d columns and the others none.  Every case runs with the path
forced, then with the window (1, 4, 8) and the run (2: at least three reduce passes at d = 67; 3 and 16: buckets of
exactly R, R + 1 and 0 entries) forced, and once more on the table path: identical bytes."""
import random

import numpy as np
import pytest

from conftest import engine_key
from test_gpu_lincomb import problem
from test_gpu_sum import ALL_KEYS, material

pytestmark = pytest.mark.gpu

SHAPES = {(1, 1, 1): 31, (1, 1, 67): 31, (2, 3, 67): 9, (1, 2, 300): 16}      # (nvec, nrows, d): w_bits
CASES = [(k, s) for k in ALL_KEYS for s in SHAPES if not (k == "k2048" and s == (1, 2, 300))]
FORCED = [("lin_bucket_window", w) for w in (1, 4, 8)] + [("lin_bucket_run", k) for k in (2, 3, 16)]
REDUCE = {1: "k_bkt_reduce_g1", 2: "k_bkt_reduce_gt"}


def equal_rows(m, level, idx, W, w_bits):
    """Every weight of row r equal to W[r][0] (reduced as the engine reduces it), and the results that belong to it."""
    W = np.repeat(W[:, :1], W.shape[1], axis=1)
    eff = np.sign(W.astype(np.int64)) * (np.abs(W.astype(np.int64)) % (1 << w_bits))
    exps = m.exp1 if level == 1 else [(e,) for e in m.exp2]
    totals = [tuple(sum(int(eff[r, j]) * exps[idx[v, j]][c] for j in range(W.shape[1])) % m.n for c in range(len(exps[0])))
              for v in range(idx.shape[0]) for r in range(W.shape[0])]
    return np.ascontiguousarray(W), m.expect(level, totals if level == 1 else [t[0] for t in totals])


@pytest.mark.parametrize("pattern", ["mixed", "equal"])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name,shape", CASES, ids=["%s-%dx%dx%d" % ((k,) + s) for k, s in CASES])
def test_the_bucket_path_gives_the_oracles_bytes_under_every_setting(name, shape, level, pattern, engopts):
    m = material(name)
    eng = engine_key(m.fx)[0].engine
    nvec, nrows, d = shape
    wb = SHAPES[shape]
    idx, W, ct, want, _ = problem(m, level, nvec, nrows, d, wb, "bkt-%s-%d-%s" % (name, level, shape))
    if pattern == "equal":
        W, want = equal_rows(m, level, idx, W, wb)
    engopts.set("lin_buckets", 1)
    got = eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes()
    assert eng.last_kernel_name() == REDUCE[level] and eng.last_aux_kernel_name() == "k_bkt_scatter"
    assert got == want, "buckets, planned window and run"
    for opt, k in FORCED:
        engopts.set(opt, k)
        assert eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes() == want, "%s = %d" % (opt, k)
        assert eng.last_kernel_name() == REDUCE[level]
        engopts.unset(opt)
    engopts.set("lin_buckets", 0)
    assert eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes() == want, "tables"
    assert eng.last_kernel_name() == ("k_lin_walk_g1" if level == 1 else "k_lin_walk_gt")


def test_blinded_bucket_maps(engopts):
    """One r per result, as test_gpu_lincomb.test_blinded_linear_maps."""
    m = material("k1024b")
    eng = engine_key(m.fx)[0].engine
    o, n = m.o, m.n
    rng = random.Random("bkt-blind")
    engopts.set("lin_buckets", 1)
    for level in (1, 2):
        _, W, ct, want, totals = problem(m, level, 2, 3, 7, 9, "bkt-blind-%d" % level)
        rs = [0] + [rng.randrange(n) for _ in range(5)]
        got = eng.lincomb(level, ct, W, w_bits=9, r=rs, nvec=2).tobytes()
        assert eng.last_kernel_name() == REDUCE[level]
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
    _, W, ct, want, _ = problem(m, level, nvec, nrows, d, 9, "bkt-dev-%d" % level)
    ct = np.frombuffer(ct, dtype=np.uint8)
    d_w = torch.from_numpy(W.copy()).cuda()
    engopts.set("lin_buckets", 1)
    for off_in, off_out in [(1, 3), (2, 1), (3, 2)]:
        d_in = torch.zeros(len(ct) + 8, dtype=torch.uint8, device="cuda")
        d_in[off_in:off_in + len(ct)] = torch.from_numpy(ct.copy()).cuda()
        d_out = torch.full((2 * G + len(want) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = G + off_out
        eng.lincomb_dev(level, d_in[off_in:], d_w, 9, d_out[lo:], nvec, nrows, d)
        torch.cuda.synchronize()
        assert eng.last_kernel_name() == REDUCE[level]
        h = d_out.cpu().numpy()
        assert h[lo:lo + len(want)].tobytes() == want, (off_in, off_out)
        assert (h[:lo] == 0xA5).all() and (h[lo + len(want):] == 0xA5).all(), (off_in, off_out)
