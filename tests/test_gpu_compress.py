"""GPU: the compressed wire form (include/bgn_amd.h; csrc/compressops.hpp) — bgn_compress_batch, bgn_decompress_batch and
their `_dev` twins against Python integers: the flag from y & 1, the root as pow(rhs, (p + 1) // 4, p).  Every limb
count (toy64 3, k256 10, k512 19, k1024 36, k1024b 37, k2048 72), both levels; counts 1, 64, 65, 257 (a lane, a wave,
a wave plus one, more than one workgroup) at k256, 3 and 65 elsewhere; the device forms at every byte offset."""
import pytest

from conftest import engine_key, load_fixture

pytestmark = pytest.mark.gpu

KEYS = ("toy64", "k256", "k512", "k1024", "k1024b", "k2048")
_INPUTS = {}
DECOMPRESS_SCRATCH_36 = 0          # bytes per lane bgn_last_kernel_resources reports for k_decompress at 36 limbs


def ints(elem, L):
    return int.from_bytes(elem[:L], "big"), int.from_bytes(elem[L:], "big")


def ref_compress(level, elem, p, L):
    a, b = ints(elem, L)
    if level == 1:
        return a.to_bytes(L, "big") + bytes([0 if a == 0 and b == 0 else 2 | (b & 1)])
    return (a % p).to_bytes(L, "big") + bytes([2 | (b % p & 1)])


def identity(level, L):
    return bytes(2 * L) if level == 1 else (1).to_bytes(L, "big") + bytes(L)


def ref_decompress(level, c, p, L):
    x, flag = int.from_bytes(c[:L], "big"), c[L]
    if level == 1 and flag == 0 and x == 0:
        return identity(1, L), 1
    if flag not in (2, 3) or x >= p or (level == 1 and x == 0):
        return identity(level, L), 0
    rhs = (x * x * x + x) % p if level == 1 else (1 - x * x) % p
    y = pow(rhs, (p + 1) // 4, p)
    if y * y % p != rhs or (y == 0 and flag == 3):
        return identity(level, L), 0
    if (y ^ flag) & 1:
        y = p - y
    return x.to_bytes(L, "big") + y.to_bytes(L, "big"), 1


def inputs(name, level):
    """257 (k256) or 65 full elements, computed once.  Level 1: oracle encryptions, the first one of (0, 0) — the
    identity.  Level 2: eng.make_l2 of them, then 1 || 0, re = p - 1 (im = 0) and a residue >= p."""
    if (name, level) not in _INPUTS:
        import oracle_c
        fx = load_fixture(name)
        eng = engine_key(fx)[0].engine
        o = oracle_c.Oracle.from_fixture(fx)
        p, L, n = eng.p, eng.L, int(fx["n"], 16)
        count = 257 if name == "k256" else 65
        l1 = o.encrypt([(7 * i) % n for i in range(count)], [(i * i * 0x9E3779B1) % n for i in range(count)])
        rows = [l1[i * 2 * L:(i + 1) * 2 * L] for i in range(count)]
        assert rows[0] == bytes(2 * L)
        if level == 2:
            rows = [bytes(r) for r in eng.make_l2(l1)]
            rows[0] = identity(2, L)
            rows[1] = (p - 1).to_bytes(L, "big") + bytes(L)
            big = next(r for r in rows[3:] if ints(r, L)[0] + p < 256 ** L)
            rows[2] = (ints(big, L)[0] + p).to_bytes(L, "big") + big[L:]
        _INPUTS[(name, level)] = (eng, p, L, rows)
    return _INPUTS[(name, level)]


def dev_compress(eng, level, a, count, off):
    import torch
    src = torch.zeros(len(a) + 8, dtype=torch.uint8, device="cuda")
    src[off:off + len(a)] = torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda()
    n = count * (eng.L + 1)
    dst = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    eng.compress_dev(level, src[off:off + len(a)], dst[(off + 1) & 3:][:n], count)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().tobytes()
    lo = (off + 1) & 3
    assert got[:lo] == bytes(lo) and got[lo + n:] == bytes(8 - lo)          # nothing written outside
    return got[lo:lo + n]


def dev_decompress(eng, level, c, count, off):
    import torch
    src = torch.zeros(len(c) + 8, dtype=torch.uint8, device="cuda")
    src[off:off + len(c)] = torch.frombuffer(bytearray(c), dtype=torch.uint8).cuda()
    n = count * 2 * eng.L
    dst = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    ok = torch.full((count + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    lo = (off + 3) & 3
    eng.decompress_dev(level, src[off:off + len(c)], dst[lo:lo + n], ok[off:off + count], count)
    torch.cuda.synchronize()
    got, okb = dst.cpu().numpy().tobytes(), ok.cpu().numpy().tobytes()
    assert got[:lo] == bytes(lo) and got[lo + n:] == bytes(8 - lo)
    assert okb[:off] == b"\x5a" * off and okb[off + count:] == b"\x5a" * (8 - off)
    return got[lo:lo + n], okb[off:off + count]


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", KEYS)
def test_compress_equals_the_reference_and_decompress_inverts_it(name, level):
    eng, p, L, rows = inputs(name, level)
    for count in (1, 64, 65, 257) if name == "k256" else (3, 65):
        a = b"".join(rows[:count])
        want = b"".join(ref_compress(level, r, p, L) for r in rows[:count])
        # the full form decompress must give back: the input, its residues reduced on level 2
        full = b"".join(ref_decompress(level, want[i * (L + 1):(i + 1) * (L + 1)], p, L)[0] for i in range(count))
        assert full == b"".join(b"".join((v % p).to_bytes(L, "big") for v in ints(r, L)) for r in rows[:count])
        got = eng.compress(level, a)
        assert eng.last_kernel_name() == "k_compress_wire"
        assert got.tobytes() == want, (name, level, count, "compress")
        back, ok = eng.decompress(level, got)
        assert eng.last_kernel_name() == "k_decompress"
        assert back.tobytes() == full and ok.tobytes() == b"\x01" * count, (name, level, count, "decompress")
        if level == 1:
            assert eng.validate(1, back).tobytes() == b"\x01" * count
        for off in range(4) if count == 65 else (count & 3,):
            assert dev_compress(eng, level, a, count, off) == want, (name, level, count, off)
            assert dev_decompress(eng, level, want, count, off) == (full, b"\x01" * count), (name, level, count, off)


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", KEYS)
def test_every_rejection_rule_among_accepted_lanes(name, level):
    eng, p, L, rows = inputs(name, level)
    good = [ref_compress(level, r, p, L) for r in rows[:65]]

    def with_flag(c, f):
        return c[:L] + bytes([f])

    bad = {}
    x = next(x for x in range(2, 1000)
             if pow((x * x * x + x) % p if level == 1 else (1 - x * x) % p, (p - 1) // 2, p) == p - 1)
    bad[5] = x.to_bytes(L, "big") + b"\x02"                     # rhs is a non-residue
    bad[9] = p.to_bytes(L, "big") + b"\x02"                     # x = p
    for i, f in ((13, 0x01), (17, 0x04), (21, 0xFF)):
        bad[i] = with_flag(good[i], f)
    if level == 1:
        bad[25] = bytes(L) + b"\x02"                            # (0, 0) spelled as a finite point
        bad[29] = bytes(L) + b"\x03"                            # ... and with a zero root's impossible parity
        bad[33] = with_flag(good[33], 0x00)                     # flag 0x00 with x != 0
    else:
        bad[25] = (1).to_bytes(L, "big") + b"\x03"              # re = 1: the root is 0, the flag says odd
        bad[29] = with_flag(good[29], 0x00)                     # flag 0x00 on level 2
        bad[33] = (p - 1).to_bytes(L, "big") + b"\x03"
    batch = [bad.get(i, c) for i, c in enumerate(good)]
    want = [ref_decompress(level, c, p, L) for c in batch]
    assert [w[1] for w in want] == [0 if i in bad else 1 for i in range(65)]
    assert all(want[i][0] == identity(level, L) for i in bad)
    got, ok = eng.decompress(level, b"".join(batch))
    assert ok.tolist() == [w[1] for w in want], (name, level)
    assert got.tobytes() == b"".join(w[0] for w in want), (name, level)
    assert dev_decompress(eng, level, b"".join(batch), 65, 1) == (got.tobytes(), ok.tobytes())
    # accepted inputs come back from compress as they went in
    keep = [i for i in range(65) if i not in bad]
    assert eng.compress(level, got[keep]).tobytes() == b"".join(batch[i] for i in keep)


def test_kernel_resources():
    """k_compress_wire is k_neg_wire's class: no scratch, no LDS beyond the stage.  k_decompress at 36 limbs: what the
    build achieved (DESIGN.md "Compressed wire forms")."""
    eng, p, L, rows = inputs("k1024", 1)
    c = eng.compress(1, b"".join(rows[:3]))
    res = eng.last_kernel_resources()
    eng.neg(1, b"".join(rows[:3]))
    assert eng.last_kernel_name() == "k_neg_wire"
    assert res["scratch_bytes_per_lane"] == 0 and res["lds_bytes_per_workgroup"] == eng.last_kernel_resources()["lds_bytes_per_workgroup"]
    eng.decompress(1, c)
    res = eng.last_kernel_resources()
    print("k_decompress<36>:", res)
    assert res["scratch_bytes_per_lane"] == DECOMPRESS_SCRATCH_36 and res["max_threads_per_workgroup"] >= 256

