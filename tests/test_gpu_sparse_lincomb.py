"""GPU: sparse linear maps (bgn_sparse_lincomb_batch / _dev; csrc/sparseops.hpp) — out[v][r] = sum over the entries e of
row r of w[e] * ct[v][col[e]], the index arrays in compressed-row form.

The method is that of test_gpu_lincomb.py on the material of test_gpu_sum.py: every ciphertext encrypts known exponents,
so a result must be the C oracle's encryption of the integer sums taken in Python — after `rows` below has applied the
rules of include/bgn_amd.h for indices outside the stated bounds (row_max, nnz, d, a decreasing row_ptr).  Every case
runs under every lin_window / lin_split: identical bytes."""
import random

import numpy as np
import pytest

import bgn_amd
from conftest import engine_key
from test_gpu_sum import material

pytestmark = pytest.mark.gpu
BGN_E_ARG = -1
SETTINGS = [(w, s) for w in (-1, 1, 4) for s in (-1, 1, 3)]


def ragged(rng, top):
    """70 rows of r mod 9 entries over 37 columns: empty rows, two waves (the second partial), unequal rows in a wave."""
    lens = [r % 9 for r in range(70)]
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.array([rng.randrange(37) for _ in range(rp[-1])])
    w = np.array([rng.choice([0, 1, -1, top, -top, 0x78 & top, 15, -8]) if rng.random() < 0.5 else rng.randint(-top, top)
                  for _ in range(rp[-1])])
    k = rng.randint(1, top)
    col[rp[5]:rp[5] + 2], w[rp[5]:rp[5] + 2] = 3, (k, k)             # equal points: a doubling inside jac_add_affine
    col[rp[7]:rp[7] + 2], w[rp[7]:rp[7] + 2] = 4, (k, -k)            # opposite points: the identity mid-run
    w[rp[8]] = 0x78 & top                                            # the carry case of the recoding
    return dict(nvec=2, d=37, rp=rp, col=col, w=w, row_max=8, ident=9)


def band(rng, top):
    """300 rows, taps (1, -2, 1) at columns r .. r + 2: two workgroups, neighbouring lanes read neighbouring columns."""
    return dict(nvec=1, d=302, rp=3 * np.arange(301), col=(np.arange(300)[:, None] + np.arange(3)).reshape(-1),
                w=np.tile([1, -2, 1], 300), row_max=3, small=True)


def long_rows(rng, top):
    """Rows of 200, 1 and 0 entries: chunk counts that do not divide a row, and chunks that come out empty."""
    return dict(nvec=1, d=50, rp=np.array([0, 200, 201, 201]), col=np.array([rng.randrange(50) for _ in range(201)]),
                w=np.array([rng.randint(-top, top) for _ in range(201)]), row_max=200, splits=(1, 3, 7))


def out_of_contract(rng, top):
    """row_max below the longest row, col == d and 0xFFFFFFFF, a decreasing row_ptr, rows that run and start past nnz."""
    col = np.array([rng.randrange(10) for _ in range(14)])
    col[1], col[4], col[13] = 10, 0xFFFFFFFF, 10
    return dict(nvec=1, d=10, rp=np.array([0, 5, 3, 9, 12, 12, 40, 45]), col=col,
                w=np.array([rng.randint(1, top) for _ in range(14)]), row_max=4)


STRUCTURES = {"ragged": ragged, "band": band, "long": long_rows, "ooc": out_of_contract}
CASES = [("toy64", s, 7) for s in STRUCTURES] + [("toy64", "ragged", 31), ("k1024", "ragged", 7), ("k1024", "band", 7),
                                                 ("k1024b", "ragged", 7)]


def rows(s):
    """The entries (col, w) of every row after the rules for out-of-contract indices."""
    rp, nnz = [int(x) for x in s["rp"]], len(s["col"])
    out = []
    for a, b in zip(rp, rp[1:]):
        n = min(b - a, s["row_max"]) if b > a else 0
        out.append([(int(s["col"][e]), int(s["w"][e])) for e in range(a, a + n) if e < nnz and s["col"][e] < s["d"]])
    return out


def problem(m, level, name, w_bits, seed):
    """The structure, the wire bytes of the vectors, the expected results and their exponent totals."""
    rng = random.Random(seed)
    s = STRUCTURES[name](rng, (1 << w_bits) - 1)
    exps = m.exp1 if level == 1 else [(e,) for e in m.exp2]
    npool = min(5, len(exps)) if s.get("small") else len(exps)         # small: few distinct totals for the oracle
    idx = np.array([[rng.randrange(npool) for _ in range(s["d"])] for _ in range(s["nvec"])])
    if "ident" in s:
        idx[:, s["ident"]] = 0                                        # an identity ciphertext
    totals = [tuple(sum(w * exps[idx[v, c]][k] for c, w in row) % m.n for k in range(len(exps[0])))
              for v in range(s["nvec"]) for row in rows(s)]
    if level == 2:
        totals = [t[0] for t in totals]
    return s, m.wire(level, idx), m.expect(level, totals), totals


def call(eng, level, s, ct, w_bits, **kw):
    return eng.sparse_lincomb(level, ct, s["rp"], s["col"], s["w"], d=s["d"], w_bits=w_bits, row_max=s["row_max"],
                              nvec=s["nvec"], **kw).tobytes()


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("key,name,w_bits", CASES, ids=["%s-%s-w%d" % c for c in CASES])
def test_sparse_maps_equal_the_oracle_under_every_setting(key, name, w_bits, level, engopts):
    m = material(key)
    eng = engine_key(m.fx)[0].engine
    s, ct, want, _ = problem(m, level, name, w_bits, "sp-%s-%s-%d-%d" % (key, name, w_bits, level))
    for window, split in SETTINGS + [(-1, k) for k in s.get("splits", ())]:
        engopts.set("lin_window", window)
        engopts.set("lin_split", split)
        assert call(eng, level, s, ct, w_bits) == want, (window, split)
        assert eng.last_kernel_name() == ("k_sp_walk_g1" if level == 1 else "k_sp_walk_gt")
    if name == "band" and key == "toy64":                             # the dense call on the densified matrix: same bytes
        W = np.zeros((300, 302), dtype=np.int32)
        W[np.repeat(np.arange(300), 3), s["col"]] = s["w"]
        assert eng.lincomb(level, ct, W, w_bits=w_bits).tobytes() == want


@pytest.mark.parametrize("level", [1, 2])
def test_blinded_sparse_maps(level):
    """One r per result: level 1 adds r to the randomness exponent, level 2 multiplies by the oracle's e(Q,Q)^r."""
    m = material("toy64")
    eng = engine_key(m.fx)[0].engine
    o, n = m.o, m.n
    rng = random.Random("sp-blind-%d" % level)
    s, ct, want, totals = problem(m, level, "ragged", 7, "sp-blind-%d" % level)
    rs = [0] + [rng.randrange(n) for _ in range(len(totals) - 1)]
    if level == 1:
        want = o.encrypt([t[0] for t in totals], [(t[1] + r) % n for t, r in zip(totals, rs)])
    else:
        Q = bytes.fromhex(m.fx["Q"])
        want = o.add(2, want, o.multconst(2, o.mult(Q, Q) * len(rs), rs))
    assert call(eng, level, s, ct, 7, r=rs) == want


@pytest.mark.parametrize("level", [1, 2])
def test_device_arrays_at_any_byte_address_and_guard_bytes(level):
    import torch
    m = material("toy64")
    eng = engine_key(m.fx)[0].engine
    s, ct, want, _ = problem(m, level, "ooc", 7, "sp-dev-%d" % level)
    ct, G = np.frombuffer(ct, dtype=np.uint8), 64
    d_rp, d_col, d_w = [torch.from_numpy(s[k].astype(np.int64).astype(np.uint32).view(np.int32)).cuda() for k in ("rp", "col", "w")]
    shape = (s["nvec"], len(s["rp"]) - 1, s["d"], len(s["col"]), s["row_max"])
    for off_in, off_out in [(1, 3), (2, 1), (3, 2)]:
        d_in = torch.zeros(len(ct) + 8, dtype=torch.uint8, device="cuda")
        d_in[off_in:off_in + len(ct)] = torch.from_numpy(ct.copy()).cuda()
        d_out = torch.full((2 * G + len(want) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = G + off_out
        eng.sparse_lincomb_dev(level, d_in[off_in:], d_rp, d_col, d_w, 7, d_out[lo:], *shape)
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        assert h[lo:lo + len(want)].tobytes() == want, (off_in, off_out)
        assert (h[:lo] == 0xA5).all() and (h[lo + len(want):] == 0xA5).all(), (off_in, off_out)
    for bad in range(3):                                               # row_ptr, col, w at an odd address
        arrs = [a if i != bad else torch.cat([a, a]).view(torch.uint8)[1:] for i, a in enumerate((d_rp, d_col, d_w))]
        with pytest.raises(bgn_amd.BgnError):
            eng.sparse_lincomb_dev(level, d_in[off_in:], *arrs, 7, d_out[lo:], *shape)


def test_bad_arguments_on_a_live_context():
    import ctypes as C
    m = material("toy64")
    eng = engine_key(m.fx)[0].engine
    lib, h = eng._lib, eng._h
    rp, col, w = (C.c_uint32 * 4)(0, 1, 2, 2), (C.c_uint32 * 2)(0, 1), (C.c_int32 * 2)(3, -4)
    ct = m.wire(1, np.array([1, 2]))
    stamp = b"\x5a" * (6 * m.E)
    out = C.create_string_buffer(stamp, len(stamp))
    r = b"\x01"
    # nvec, nrows, d, nnz, row_max, level, ct, row_ptr, col, w, w_bits, r, r_len, out
    good = (2, 3, 1, 2, 1, 1, ct, rp, col, w, 9, None, 0, out)
    for at, v in [(0, 0), (1, 0)]:                                     # nvec == 0, nrows == 0: nothing to do
        assert lib.bgn_sparse_lincomb_batch(h, *(good[:at] + (v,) + good[at + 1:])) == 0
    for at, v in [(2, 0), (4, 0), (5, 0), (5, 3), (10, 0), (10, 32), (6, None), (7, None), (8, None), (9, None), (13, None),
                  (11, r), (0, 1 << 29), (1, 1 << 29), (3, (1 << 28) + 1), (2, 1 << 28), (0, 1 << 62)]:
        args = good[:at] + (v,) + good[at + 1:]
        assert lib.bgn_sparse_lincomb_batch(h, *args) == BGN_E_ARG, (at, v)
        assert lib.bgn_sparse_lincomb_batch_dev(h, *args, None) == BGN_E_ARG, (at, v)
    big = good[:1] + (1 << 20,) + good[2:3] + (1 << 20, 1 << 10) + good[5:]      # nrows * min(row_max, nnz) = 2^30
    assert lib.bgn_sparse_lincomb_batch(h, *big) == BGN_E_ARG
    assert out.raw == stamp
