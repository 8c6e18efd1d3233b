"""GPU: segmented sums (bgn_sum_batch / bgn_sum_batch_dev; csrc/sumops.hpp) — out[s] = ct[s*seg_len] + ... — the
loop of Add the reference folds an array with (bgn.go:442-497; gadgets_test.go:24-46).

Expected values never come from the engine: every element is an encryption of known exponents (level 1: P^x Q^r;
level 2: g^k with g = e(P, P) from ONE oracle pairing per key), so the sum of a segment is the C oracle's encryption
of the exponent sums — one exponentiation per segment, whatever order the engine accumulates in.  The exponents come
from a small pool (0, 1, 2, n-1, n-2), so identities, equal points (a doubling inside the mixed addition) and opposite
points (the identity mid-run) meet the accumulators at many positions; one segment is all identities and one sums to
the identity.  Every shape runs planned and — the multi-element ones — with the first pass's split forced to 1 (a lone
lane per segment), 7 (does not divide the lengths) and 64 (more than one pass): identical bytes each time."""
import random

import numpy as np
import pytest

import bgn_amd.synthetic as syn
from conftest import engine_key, load_fixture

pytestmark = pytest.mark.gpu

ALL_KEYS = ["toy64", "k256", "k512", "k1024", "k1024b", "k2048"]
BASE_SHAPES = [(1, 1), (1, 2), (1, 63), (3, 65), (257, 1), (65, 4), (1, 257)]
EXTRA = {"toy64": [(2, 1000), (1, 5000)], "k256": [(2, 1000), (1, 5000)], "k512": [(2, 1000), (1, 5000)],
         "k1024": [(1, 1000)]}
CASES = [(k, s) for k in ALL_KEYS for s in BASE_SHAPES + EXTRA.get(k, [])]
FORCED = (1, 7, 64)
BGN_E_ARG = -1


def test_the_keys_cover_every_limb_count():
    assert {syn.limbs_for(int(load_fixture(k)["p"], 16)) for k in ALL_KEYS} == {3, 10, 19, 36, 37, 72}


class Material:
    """Per key: the oracle, the pools of both levels (exponents and their wire bytes) and a cache of expected sums."""

    def __init__(self, name):
        import oracle_c
        self.fx = fx = load_fixture(name)
        self.o = o = oracle_c.Oracle.from_fixture(fx)
        self.n = n = int(fx["n"], 16)
        self.E = o.E
        rng = random.Random("sum-" + name)
        # level 1: (x, r); the first five are the small pool with r = 0, the rest random pairs
        self.exp1 = [(0, 0), (1, 0), (2, 0), (n - 1, 0), (n - 2, 0)] + [(rng.randrange(n), rng.randrange(n)) for _ in range(12)]
        w = o.encrypt([e[0] for e in self.exp1], [e[1] for e in self.exp1])
        self.pool1 = np.frombuffer(w, dtype=np.uint8).reshape(len(self.exp1), self.E)
        assert not self.pool1[0].any()                                   # P^0 Q^0: the all-zero identity
        # level 2: g^k
        one = o.encrypt([1])
        self.g = o.mult(one, one)
        self.exp2 = [0, 1, 2, n - 1]
        w = o.multconst(2, self.g * len(self.exp2), self.exp2)
        self.pool2 = np.frombuffer(w, dtype=np.uint8).reshape(len(self.exp2), self.E)
        self.one2 = (1).to_bytes(self.E // 2, "big") + bytes(self.E // 2)
        assert self.pool2[0].tobytes() == self.one2                      # g^0 = 1 || 0
        self.cache = {}
        self.eqq = None

    def expect(self, level, totals):
        """Wire bytes of the sums with these exponent totals (level 1: (x, r) pairs; level 2: k)."""
        miss = [t for t in dict.fromkeys(totals) if (level, t) not in self.cache]
        if miss:
            if level == 1:
                w = self.o.encrypt([t[0] for t in miss], [t[1] for t in miss])
            else:
                w = self.o.multconst(2, self.g * len(miss), miss)
            for i, t in enumerate(miss):
                self.cache[(level, t)] = w[i * self.E:(i + 1) * self.E]
        return b"".join(self.cache[(level, t)] for t in totals)

    def content(self, level, nseg, seg_len, seed):
        """Pool indices (nseg x seg_len) and the exponent total of every segment."""
        rng = random.Random(seed)
        n = self.n
        idx = np.zeros((nseg, seg_len), dtype=np.int64)
        for s in range(nseg):
            if level == 1:
                # every eighth segment also draws the random pairs (their totals cost two full exponentiations each)
                hi = len(self.exp1) if s % 8 == 0 else 5
                row = [rng.randrange(hi) for _ in range(seg_len)]
            else:
                row = rng.choices(range(4), weights=[25, 40, 30, 5], k=seg_len)
            idx[s] = row
        if nseg >= 2:                                    # a segment whose total is the identity: 1 + (n-1) + ... (+ 0)
            pair = [1, 3]
            idx[1] = [pair[j % 2] for j in range(seg_len - seg_len % 2)] + [0] * (seg_len % 2)
        if nseg >= 3:                                    # a segment of identities
            idx[2] = 0
        if level == 1:
            totals = [(sum(self.exp1[i][0] for i in row) % n, sum(self.exp1[i][1] for i in row) % n) for row in idx]
        else:
            totals = [sum(self.exp2[i] for i in row) % n for row in idx]
        if nseg >= 2:
            assert totals[1] == ((0, 0) if level == 1 else 0)
        return idx, totals

    def wire(self, level, idx):
        pool = self.pool1 if level == 1 else self.pool2
        return pool[idx.reshape(-1)].reshape(-1).tobytes()


_MAT = {}


def material(name):
    if name not in _MAT:
        _MAT[name] = Material(name)
    return _MAT[name]


def kernel_of(level):
    return "k_sum_g1_wire" if level == 1 else "k_sum_gt_wire"


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name,shape", CASES, ids=["%s-%dx%d" % (k, s[0], s[1]) for k, s in CASES])
def test_sums_equal_the_oracle_for_every_split(name, shape, level, engopts):
    m = material(name)
    pk, _ = engine_key(m.fx)
    eng = pk.engine
    nseg, seg_len = shape
    idx, totals = m.content(level, nseg, seg_len, "%s-%d-%d-%d" % (name, level, nseg, seg_len))
    ct = m.wire(level, idx)
    want = m.expect(level, totals)
    got = eng.sum(level, ct, seg_len).tobytes()
    assert eng.last_kernel_name() == kernel_of(level)
    assert got == want, "planned"
    if nseg >= 3:
        ident = bytes(m.E) if level == 1 else m.one2
        assert got[m.E:2 * m.E] == ident and got[2 * m.E:3 * m.E] == ident
    if seg_len > 1:
        for k in FORCED:
            engopts.set("sum_split", k)
            assert eng.sum(level, ct, seg_len).tobytes() == want, "sum_split = %d" % k
        engopts.unset("sum_split")


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ALL_KEYS)
def test_device_arrays_at_any_byte_address_and_guard_bytes(name, level):
    """ct and out at byte offsets 0..3 of their allocations; the bytes around out stay what they were."""
    import torch
    m = material(name)
    pk, _ = engine_key(m.fx)
    eng = pk.engine
    nseg, seg_len, G = 3, 65, 64
    idx, totals = m.content(level, nseg, seg_len, "dev-%s-%d" % (name, level))
    ct = np.frombuffer(m.wire(level, idx), dtype=np.uint8)
    want = m.expect(level, totals)
    for off_in, off_out in [(0, 0), (1, 3), (2, 1), (3, 2), (0, 2), (2, 0)]:
        d_in = torch.zeros(len(ct) + 8, dtype=torch.uint8, device="cuda")
        d_in[off_in:off_in + len(ct)] = torch.from_numpy(ct.copy()).cuda()
        d_out = torch.full((2 * G + nseg * m.E + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = G + off_out
        eng.sum_dev(level, d_in[off_in:], d_out[lo:], nseg, seg_len)
        torch.cuda.synchronize()
        assert eng.last_kernel_name() == kernel_of(level)
        h = d_out.cpu().numpy()
        assert h[lo:lo + nseg * m.E].tobytes() == want, (off_in, off_out)
        assert (h[:lo] == 0xA5).all() and (h[lo + nseg * m.E:] == 0xA5).all(), (off_in, off_out)
    res = eng.last_kernel_resources()
    assert res["max_threads_per_workgroup"] >= 128 and res["lds_bytes_per_workgroup"] <= 160 * 1024


@pytest.mark.parametrize("name", ["toy64", "k256", "k1024b"])
def test_blinded_sums(name):
    """One r per segment: level 1 adds r to the randomness exponent, level 2 multiplies by the oracle's e(Q,Q)^r."""
    m = material(name)
    pk, _ = engine_key(m.fx)
    eng = pk.engine
    o, n = m.o, m.n
    rng = random.Random("blind-" + name)
    for level, (nseg, seg_len) in [(1, (5, 9)), (2, (5, 9)), (1, (2, 1)), (2, (1, 300))]:
        idx, totals = m.content(level, nseg, seg_len, "blind-%s-%d-%d" % (name, level, seg_len))
        rs = [rng.randrange(n) for _ in range(nseg)]
        rs[0] = 0
        got = eng.sum(level, m.wire(level, idx), seg_len, r=rs).tobytes()
        if level == 1:
            want = o.encrypt([t[0] for t in totals], [(t[1] + r) % n for t, r in zip(totals, rs)])
        else:
            if m.eqq is None:
                Q = bytes.fromhex(m.fx["Q"])
                m.eqq = o.mult(Q, Q)
            want = o.add(2, m.expect(2, totals), o.multconst(2, m.eqq * nseg, rs))
        assert got == want, (level, nseg, seg_len)


def test_public_key_sum_and_sum_batch():
    import bgn_amd
    from bgn_amd import Ciphertext
    m = material("k256")
    fx = m.fx
    pk, _ = engine_key(fx)
    for level in (1, 2):
        idx, totals = m.content(level, 4, 6, "pk-%d" % level)
        pool = m.pool1 if level == 1 else m.pool2
        rows = [[Ciphertext(pool[i].tobytes(), level == 2) for i in row] for row in idx]
        want = m.expect(level, totals)
        got = pk.SumBatch(rows)
        assert b"".join(c.C for c in got) == want and all(c.L2 == (level == 2) for c in got)
        assert pk.Sum(rows[0]).C == want[:m.E]
    assert pk.SumBatch([]) == []
    mixed = [[Ciphertext(m.pool1[1].tobytes(), False), Ciphertext(m.pool2[1].tobytes(), True)]]
    with pytest.raises(ValueError):
        pk.SumBatch(mixed)
    with pytest.raises(ValueError):
        pk.SumBatch([[mixed[0][0]], [mixed[0][0], mixed[0][0]]])
    # a key that blinds: explicit r through Engine.sum is the oracle's; Sum draws its own r and is a valid ciphertext
    pk2 = bgn_amd.PublicKey(int(fx["p"], 16), int(fx["n"], 16), fx["l"], bytes.fromhex(fx["P"]), bytes.fromhex(fx["Q"]),
                            fx["msg_space"], False, fx["poly_base"])
    try:
        idx, totals = m.content(1, 2, 5, "pk2")
        rs = [12345, m.n - 7]
        got = pk2.engine.sum(1, m.wire(1, idx), 5, r=rs).tobytes()
        assert got == m.o.encrypt([t[0] for t in totals], [(t[1] + r) % m.n for t, r in zip(totals, rs)])
        rows = [[Ciphertext(m.pool1[i].tobytes(), False) for i in row] for row in idx]
        blinded = pk2.SumBatch(rows)
        assert b"".join(c.C for c in blinded) != m.expect(1, totals)
        assert pk2.engine.validate(1, b"".join(c.C for c in blinded)).tolist() == [1, 1]
    finally:
        pk2.engine.close()


def test_bad_arguments_on_a_live_context():
    import ctypes as C
    m = material("toy64")
    pk, _ = engine_key(m.fx)
    eng = pk.engine
    lib, h = eng._lib, eng._h
    ct = m.wire(1, m.content(1, 2, 3, "arg")[0])
    out = C.create_string_buffer(2 * m.E)
    stamp = b"\x5a" * (2 * m.E)
    out.raw = stamp
    assert lib.bgn_sum_batch(h, 0, 3, 1, None, None, 0, None) == 0                    # nseg == 0
    for args in [(2, 0, 1, ct, None, 0, out), (2, 3, 0, ct, None, 0, out), (2, 3, 3, ct, None, 0, out),
                 (2, 3, 1, None, None, 0, out), (2, 3, 1, ct, None, 0, None), (2, 3, 1, ct, b"\x01\x01", 0, out),
                 (1 << 20, 1 << 9, 1, ct, None, 0, out), (1 << 40, 1 << 40, 1, ct, None, 0, out)]:
        assert lib.bgn_sum_batch(h, *args) == BGN_E_ARG, args[:3]
        assert lib.bgn_sum_batch_dev(h, *args, None) == BGN_E_ARG, args[:3]
    assert out.raw == stamp
    with pytest.raises(ValueError):
        eng.sum(1, ct, 4)                                                             # 6 elements, segments of 4
