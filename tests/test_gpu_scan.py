"""GPU: prefix sums (bgn_scan_batch; csrc/scanops.hpp).  Expected values never come from the engine: the elements are
the small-exponent pool entries of test_gpu_sum's material, so prefix i is the C oracle's encryption of the cumulative
exponent, cached by value.  Segment 0 starts 1, 1, 2 (prefix == next element: doublings), segment 1 alternates 1 and
n-1 (every second prefix IS the identity), segment 2 is all identities.  Every shape runs planned, with the first
level's chunk forced to 2, 7 and 64, and on level 1 with the apply launches cut into ranges: identical bytes."""
import random

import numpy as np
import pytest

from conftest import engine_key
from test_gpu_sum import ALL_KEYS, material

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (3, 65), (257, 1), (2, 130)]
CASES = [(k, s) for k in ALL_KEYS for s in SHAPES + ([(1, 600)] if k in ("toy64", "k256", "k512") else [])]
STEP = {1: [0, 1, 2, -1, -2], 2: [0, 1, 2, -1]}          # the pools' exponents as steps of the walk
KERNEL = {1: "k_scan_g1_wire", 2: "k_scan_gt_wire"}


def content(m, level, nseg, seg_len, seed):
    """Wire bytes of nseg x seg_len pool elements and of their prefixes."""
    rng = random.Random(seed)
    step = STEP[level]
    idx = np.zeros((nseg, seg_len), dtype=np.int64)
    for s in range(nseg):
        t = 0
        for j in range(seg_len):
            i = rng.randrange(len(step))
            while abs(t + step[i]) > 6:
                i = rng.randrange(len(step))
            idx[s, j] = i
            t += step[i]
    idx[0, :3] = [1, 1, 2][:seg_len]
    if nseg >= 2:
        idx[1] = [[1, 3][j % 2] for j in range(seg_len)]
    if nseg >= 3:
        idx[2] = 0
    run = np.cumsum(np.array(step)[idx], axis=1).reshape(-1)
    totals = [(int(t) % m.n, 0) if level == 1 else int(t) % m.n for t in run]
    pool = m.pool1 if level == 1 else m.pool2
    return pool[idx.reshape(-1)].reshape(-1).tobytes(), m.expect(level, totals), totals


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name,shape", CASES, ids=["%s-%dx%d" % (k, s[0], s[1]) for k, s in CASES])
def test_prefixes_equal_the_oracle_under_every_chunk(name, shape, level, engopts):
    m = material(name)
    eng = engine_key(m.fx)[0].engine
    nseg, seg_len = shape
    ct, want, _ = content(m, level, nseg, seg_len, "scan-%s-%d-%d-%d" % (name, level, nseg, seg_len))
    got = eng.scan(level, ct, seg_len).tobytes()
    assert eng.last_kernel_name() == KERNEL[level]
    assert got == want, "planned"
    for k in (2, 7, 64):
        engopts.set("scan_chunk", k)
        assert eng.scan(level, ct, seg_len).tobytes() == want, "scan_chunk = %d" % k
    if level == 1:                       # 600 -> 300 lanes, 257 x 1 -> 257, and at 128 threads 2 x 130 -> 130: more than a workgroup
        engopts.set("scan_chunk", 2)
        engopts.set("scan_range", 1)
        assert eng.scan(level, ct, seg_len).tobytes() == want, "ranges of one workgroup"
    engopts.unset("scan_chunk")
    engopts.unset("scan_range")


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ALL_KEYS)
def test_device_arrays_at_any_byte_address_and_guard_bytes(name, level, engopts):
    """ct and out at byte offsets 0..3; the bytes around out stay.  Chunks of 7: rows sharing a dword meet in both ways."""
    import torch
    m = material(name)
    eng = engine_key(m.fx)[0].engine
    nseg, seg_len, G = 3, 65, 64
    ct, want, _ = content(m, level, nseg, seg_len, "dev-%s-%d" % (name, level))
    engopts.set("scan_chunk", 7)
    for off_in, off_out in [(0, 0), (1, 3), (2, 1), (3, 2), (0, 2), (2, 0)]:
        d_in = torch.zeros(len(ct) + 8, dtype=torch.uint8, device="cuda")
        d_in[off_in:off_in + len(ct)] = torch.frombuffer(bytearray(ct), dtype=torch.uint8).cuda()
        d_out = torch.full((2 * G + len(want) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        lo = G + off_out
        eng.scan_dev(level, d_in[off_in:], d_out[lo:], nseg, seg_len)
        torch.cuda.synchronize()
        assert eng.last_kernel_name() == KERNEL[level]
        h = d_out.cpu().numpy()
        assert h[lo:lo + len(want)].tobytes() == want, (off_in, off_out)
        assert (h[:lo] == 0xA5).all() and (h[lo + len(want):] == 0xA5).all(), (off_in, off_out)


def test_blinded_prefixes_and_the_public_key_calls():
    """One r per OUTPUT: level 1 adds r to the randomness exponent, level 2 multiplies by the oracle's e(Q,Q)^r."""
    from bgn_amd import Ciphertext
    for name in ("toy64", "k256"):
        m = material(name)
        pk = engine_key(m.fx)[0]
        o, n = m.o, m.n
        rng = random.Random("scan-blind-" + name)
        for level, (nseg, seg_len) in [(1, (2, 9)), (2, (2, 9)), (1, (3, 1))]:
            ct, want, totals = content(m, level, nseg, seg_len, "blind-%s-%d-%d" % (name, level, seg_len))
            rs = [0] + [rng.randrange(n) for _ in range(nseg * seg_len - 1)]
            got = pk.engine.scan(level, ct, seg_len, r=rs).tobytes()
            if level == 1:
                want = o.encrypt([t[0] for t in totals], rs)
            else:
                m.eqq = m.eqq or o.mult(bytes.fromhex(m.fx["Q"]), bytes.fromhex(m.fx["Q"]))
                want = o.add(2, want, o.multconst(2, m.eqq * len(rs), rs))
            assert got == want, (name, level, nseg, seg_len)
    for level in (1, 2):                                     # (m, pk: k256)
        ct, want, _ = content(m, level, 4, 6, "pk-%d" % level)
        rows = [[Ciphertext(ct[(s * 6 + j) * m.E:(s * 6 + j + 1) * m.E], level == 2) for j in range(6)] for s in range(4)]
        got = pk.ScanBatch(rows)
        assert b"".join(c.C for r in got for c in r) == want and all(c.L2 == (level == 2) for r in got for c in r)
        assert b"".join(c.C for c in pk.Scan(rows[1])) == want[6 * m.E:12 * m.E]
