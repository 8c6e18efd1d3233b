"""GPU: linear maps of ciphertext vectors (bgn_lincomb_batch / _dev; csrc/linops.hpp) — out[v][r] = sum_j W[r][j] * ct[v][j].

The method is that of test_gpu_sum.py, whose per-key material is reused: every ciphertext is an encryption of known
exponents, so out[v][r] must be the C oracle's encryption of sum W*x, sum W*r mod n (level 1) resp. g^(sum W*k mod n)
(level 2), the sums taken in Python integers.  The weights are drawn from the values that exercise the recoding (0, +-1,
+-(2^w_bits - 1), +-2^(omega-1) and +-(2^omega - 1) for omega = 2, 4, 8, a weight above 2^w_bits); row 0 is all zero,
row 1 is (+k, -k) on two copies of one ciphertext (the identity mid-run), row 2 has equal weights on them (a doubling
inside the mixed addition); the last ciphertext of a vector is the identity.  Every case runs planned and with the
window and the split forced: identical bytes."""
import random

import numpy as np
import pytest

import bgn_amd
from conftest import engine_key
from test_gpu_sum import ALL_KEYS, material

pytestmark = pytest.mark.gpu

SHAPES = {(1, 1, 1): 31, (1, 65, 1): 9, (1, 1, 65): 31, (2, 3, 7): 9, (1, 65, 33): 16}      # (nvec, nrows, d): w_bits
CASES = [(k, s) for k in ALL_KEYS for s in SHAPES if not (k == "k2048" and s == (1, 65, 33))]
FORCED = [("lin_window", w) for w in (1, 2, 4, 8)] + [("lin_split", k) for k in (1, 3)]
BGN_E_ARG = -1


def problem(m, level, nvec, nrows, d, w_bits, seed):
    """Pool indices (nvec x d), weights (nrows x d), the wire bytes of the vectors and the expected results."""
    rng = random.Random(seed)
    top = (1 << w_bits) - 1
    special = [0, 1, -1, top, -top] + [s * v for v in (2, 3, 8, 15, 128, 255) for s in (1, -1)]
    if w_bits < 31:
        special += [(1 << w_bits) + 5, -(1 << w_bits) - 5]              # counts as +-5
    npool = len(m.exp1) if level == 1 else len(m.exp2)
    idx = np.array([[rng.randrange(npool) for _ in range(d)] for _ in range(nvec)])
    if d >= 2:
        idx[:, 1] = idx[:, 0]                                            # two copies of one ciphertext
    if d >= 3:
        idx[:, d - 1] = 0                                                # an identity ciphertext
    W = np.array([[rng.choice(special) if rng.random() < 0.5 else rng.randint(-top, top) for _ in range(d)]
                  for _ in range(nrows)], dtype=np.int64)
    k = rng.randint(1, top)
    if nrows >= 3:
        W[0] = 0
        W[2, :2] = k
    if d >= 2:
        W[min(1, nrows - 1), :2] = (k, -k)
    eff = np.sign(W) * (np.abs(W) % (1 << w_bits))
    exps = m.exp1 if level == 1 else [(e,) for e in m.exp2]
    totals = [tuple(sum(int(eff[r, j]) * exps[idx[v, j]][c] for j in range(d)) % m.n for c in range(len(exps[0])))
              for v in range(nvec) for r in range(nrows)]
    if level == 2:
        totals = [t[0] for t in totals]
    return idx, W.astype(np.int32), m.wire(level, idx), m.expect(level, totals), totals


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name,shape", CASES, ids=["%s-%dx%dx%d" % ((k,) + s) for k, s in CASES])
def test_linear_maps_equal_the_oracle_under_every_setting(name, shape, level, engopts):
    m = material(name)
    eng = engine_key(m.fx)[0].engine
    nvec, nrows, d = shape
    wb = SHAPES[shape]
    _, W, ct, want, _ = problem(m, level, nvec, nrows, d, wb, "lin-%s-%d-%s" % (name, level, shape))
    got = eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes()
    assert eng.last_kernel_name() == ("k_lin_walk_g1" if level == 1 else "k_lin_walk_gt")
    assert got == want, "planned"
    if nrows >= 3:
        assert got[:m.E] == (bytes(m.E) if level == 1 else m.one2)      # the row of zeros
    for opt, k in FORCED:
        engopts.set(opt, k)
        assert eng.lincomb(level, ct, W, w_bits=wb, nvec=nvec).tobytes() == want, "%s = %d" % (opt, k)
        engopts.unset(opt)
    if shape == (2, 3, 7):
        assert "k_lin_table" in eng.last_aux_kernel_name() or "k_lin_digits" == eng.last_aux_kernel_name()


@pytest.mark.parametrize("name", ["toy64", "k1024b"])
def test_blinded_linear_maps(name):
    """One r per result: level 1 adds r to the randomness exponent, level 2 multiplies by the oracle's e(Q,Q)^r."""
    m = material(name)
    eng = engine_key(m.fx)[0].engine
    o, n = m.o, m.n
    rng = random.Random("lin-blind-" + name)
    for level in (1, 2):
        _, W, ct, want, totals = problem(m, level, 2, 3, 7, 9, "lin-blind-%s-%d" % (name, level))
        rs = [0] + [rng.randrange(n) for _ in range(5)]
        got = eng.lincomb(level, ct, W, w_bits=9, r=rs, nvec=2).tobytes()
        if level == 1:
            want = o.encrypt([t[0] for t in totals], [(t[1] + r) % n for t, r in zip(totals, rs)])
        else:
            if m.eqq is None:
                Q = bytes.fromhex(m.fx["Q"])
                m.eqq = o.mult(Q, Q)
            want = o.add(2, want, o.multconst(2, m.eqq * 6, rs))
        assert got == want, level


@pytest.mark.parametrize("level", [1, 2])
def test_device_arrays_at_any_byte_address_and_guard_bytes(level):
    import torch
    m = material("k256")
    eng = engine_key(m.fx)[0].engine
    nvec, nrows, d, G = 2, 3, 7, 64
    _, W, ct, want, _ = problem(m, level, nvec, nrows, d, 9, "lin-dev-%d" % level)
    ct = np.frombuffer(ct, dtype=np.uint8)
    d_w = torch.from_numpy(W.copy()).cuda()
    for off_in, off_out in [(1, 3), (2, 1), (3, 2)]:
        d_in = torch.zeros(len(ct) + 8, dtype=torch.uint8, device="cuda")
        d_in[off_in:off_in + len(ct)] = torch.from_numpy(ct.copy()).cuda()
        d_out = torch.full((2 * G + len(want) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = G + off_out
        eng.lincomb_dev(level, d_in[off_in:], d_w, 9, d_out[lo:], nvec, nrows, d)
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        assert h[lo:lo + len(want)].tobytes() == want, (off_in, off_out)
        assert (h[:lo] == 0xA5).all() and (h[lo + len(want):] == 0xA5).all(), (off_in, off_out)
    with pytest.raises(bgn_amd.BgnError):                                     # w at an odd address
        eng.lincomb_dev(level, d_in[off_in:], d_w.view(torch.uint8).reshape(-1)[1:], 9, d_out[lo:], nvec, nrows - 1, d)


def test_public_key_lincomb():
    from bgn_amd import Ciphertext
    m = material("k256")
    pk, _ = engine_key(m.fx)
    for level in (1, 2):
        idx, W, _, want, _ = problem(m, level, 1, 3, 7, 9, "lin-pk-%d" % level)
        pool = m.pool1 if level == 1 else m.pool2
        cts = [Ciphertext(pool[i].tobytes(), level == 2) for i in idx[0]]
        Wfit = np.sign(W) * (np.abs(W) % 512)                            # LinCombBatch derives w_bits from the weights
        got = pk.LinCombBatch(Wfit, cts)
        assert b"".join(c.C for c in got) == want and all(c.L2 == (level == 2) for c in got)
        assert pk.LinComb(Wfit[1], cts).C == want[m.E:2 * m.E]
    mixed = [Ciphertext(m.pool1[1].tobytes(), False), Ciphertext(m.pool2[1].tobytes(), True)]
    for bad_w, bad_c in [([[1, 2]], mixed), ([[1, 2, 3]], mixed[:1] * 2), ([1, 2], mixed[:1] * 2), ([[1]], [])]:
        with pytest.raises(ValueError):
            pk.LinCombBatch(bad_w, bad_c)


def test_bad_arguments_on_a_live_context():
    import ctypes as C
    m = material("toy64")
    eng = engine_key(m.fx)[0].engine
    lib, h = eng._lib, eng._h
    _, W, ct, _, _ = problem(m, 1, 2, 3, 7, 9, "lin-arg")
    w = W.ctypes.data_as(C.c_void_p)
    stamp = b"\x5a" * (6 * m.E)
    out = C.create_string_buffer(stamp, len(stamp))
    assert lib.bgn_lincomb_batch(h, 0, 3, 7, 1, None, None, 9, None, 0, None) == 0          # nvec == 0
    assert lib.bgn_lincomb_batch(h, 2, 0, 7, 1, None, None, 9, None, 0, None) == 0          # nrows == 0
    for args in [(2, 3, 0, 1, ct, w, 9, None, 0, out), (2, 3, 7, 0, ct, w, 9, None, 0, out), (2, 3, 7, 3, ct, w, 9, None, 0, out),
                 (2, 3, 7, 1, ct, w, 0, None, 0, out), (2, 3, 7, 1, ct, w, 32, None, 0, out), (2, 3, 7, 1, None, w, 9, None, 0, out),
                 (2, 3, 7, 1, ct, None, 9, None, 0, out), (2, 3, 7, 1, ct, w, 9, None, 0, None), (2, 3, 7, 1, ct, w, 9, b"\x01", 0, out),
                 (1 << 20, 3, 1 << 9, 1, ct, w, 9, None, 0, out), (1 << 20, 1 << 9, 7, 1, ct, w, 9, None, 0, out),
                 (2, 1 << 20, 1 << 9, 1, ct, w, 9, None, 0, out), (1 << 40, 1 << 40, 1 << 40, 1, ct, w, 9, None, 0, out)]:
        assert lib.bgn_lincomb_batch(h, *args) == BGN_E_ARG, args[:4]
        assert lib.bgn_lincomb_batch_dev(h, *args, None) == BGN_E_ARG, args[:4]
    assert out.raw == stamp
