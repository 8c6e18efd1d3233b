"""GPU: blinding randomness expanded on the device from a 32-byte seed (include/bgn_amd.h "Randomness from a seed",
csrc/randexp.hpp) — bgn_random_scalars_batch, bgn_encrypt_seeded_batch, their `_dev` twins and the multi-device Encrypt
against hashlib and Python integers (tests/randexp_oracle.py), never against the engine itself.

Keys: the fixture keys toy64 (3 limbs), k256 (10), k1024b (37) and k2048 (72), and the seeded keys of
tests/test_gpu_proofs.py — k128s and k232s (10 limbs), k512s (19), k1024s (36, under a memory budget).  The order of
k128s has 16 bytes, so its W is exactly one block; W ends inside a block for the others.  Counts 1, 63, 65, 257: one
lane, a wave less one, a wave plus one, more than one workgroup."""
import random

import pytest

import randexp_oracle as X
from conftest import engine_key, load_fixture
from test_gpu_proofs import key

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 65, 257)
FIXTURE_KEYS = ("toy64", "k256", "k1024b", "k2048")
SEEDED_KEYS = ("k128s", "k232s", "k512s", "k1024s")
NL = {"toy64": 3, "k256": 10, "k1024b": 37, "k2048": 72, "k128s": 10, "k232s": 10, "k512s": 19, "k1024s": 36}
SEED = bytes(range(7, 39))


def engine(name):
    return engine_key(load_fixture(name))[0].engine if name in FIXTURE_KEYS else key(name)[2].engine


_WANT = {}


def want_rows(name, K, t, first, count):
    """The oracle's rows, computed once per (key, seed, stream, index range)."""
    k = (name, K, t, first, count)
    if k not in _WANT:
        _WANT[k] = X.rows(K, t, first, count, engine(name).n)
    return _WANT[k]


def test_the_keys_cover_every_limb_count():
    import bgn_amd  # noqa: F401
    for name in FIXTURE_KEYS + SEEDED_KEYS:
        eng = engine(name)
        need = (eng.p.bit_length() + 9 + 28) // 29
        assert min(nl for nl in (3, 10, 19, 36, 37, 72) if nl >= need) == NL[name], name
        assert eng.n_len == X.n_len_of(eng.n)
    assert set(NL.values()) == {3, 10, 19, 36, 37, 72}
    ends = {(engine(name).n_len + X.SURPLUS) % 32 == 0 for name in NL}
    assert ends == {True, False}                        # W ends on a block boundary (k128s), and inside a block


@pytest.mark.parametrize("name", FIXTURE_KEYS + SEEDED_KEYS)
def test_random_scalars_equal_the_oracle_on_host_and_device_arrays(name):
    import torch
    eng = engine(name)
    nl = eng.n_len
    for count in COUNTS:
        want = want_rows(name, SEED, 5, 0, count)
        assert eng.random_scalars(count, SEED, 5, 0).tobytes() == want, (name, count, "host")
        for off in range(4) if count in (1, 65) else (count & 3,):
            buf = torch.zeros(count * nl + 8, dtype=torch.uint8, device="cuda")
            eng.random_scalars_dev(buf[off:off + count * nl], count, SEED, 5, 0)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().tobytes()
            assert got[off:off + count * nl] == want, (name, count, off)
            assert got[:off] == bytes(off) and got[off + count * nl:] == bytes(8 - off)      # nothing written outside
    assert eng.last_kernel_name() == "k_random_scalars"


@pytest.mark.parametrize("name", ["toy64", "k128s", "k1024s"])
def test_indices_and_stream_ids_beyond_32_bits(name):
    eng = engine(name)
    first = (1 << 32) - 2                               # the rows straddle 2^32: a 32-bit index would wrap
    assert eng.random_scalars(5, SEED, 1, first).tobytes() == want_rows(name, SEED, 1, first, 5)
    t = (0x9E3779B9 << 32) | 3                          # a non-zero high word
    assert eng.random_scalars(3, SEED, t, 0).tobytes() == want_rows(name, SEED, t, 0, 3)
    assert want_rows(name, SEED, t, 0, 3) != want_rows(name, SEED, 3, 0, 3)
    last = (1 << 64) - 3                                # the last three indices there are
    assert eng.random_scalars(3, SEED, (1 << 64) - 1, last).tobytes() == want_rows(name, SEED, (1 << 64) - 1, last, 3)
    with pytest.raises(Exception):
        eng.random_scalars(4, SEED, 0, last)            # first_index + count past 2^64: BGN_E_ARG
    # another seed, other rows
    other = bytes(32)
    assert eng.random_scalars(3, other, 0, 0).tobytes() == want_rows(name, other, 0, 0, 3) != want_rows(name, SEED, 0, 0, 3)


@pytest.mark.parametrize("name", ["toy64", "k512s"])
def test_a_slice_of_a_call_equals_a_call_from_that_index(name):
    eng = engine(name)
    nl = eng.n_len
    whole = eng.random_scalars(257, SEED, 5, 0).tobytes()
    for a, b in ((0, 1), (63, 65), (64, 257), (200, 257)):
        assert eng.random_scalars(b - a, SEED, 5, a).tobytes() == whole[a * nl:b * nl], (name, a, b)


@pytest.mark.parametrize("name", FIXTURE_KEYS + SEEDED_KEYS)
def test_rows_are_distinct_and_below_n(name):
    eng = engine(name)
    nl = eng.n_len
    got = eng.random_scalars(257, SEED, 5, 0).tobytes()
    rows = [int.from_bytes(got[i * nl:(i + 1) * nl], "big") for i in range(257)]
    assert len(set(rows)) == 257 and all(0 <= r < eng.n for r in rows)


@pytest.mark.parametrize("name", ["toy64", "k128s", "k512s", "k1024s"])
def test_encrypt_seeded_equals_encrypt_with_the_oracles_rows(name):
    import torch
    eng = engine(name)
    nl, E = eng.n_len, eng.elem_bytes
    rng = random.Random(NL[name])
    for count in COUNTS if name != "k1024s" else (1, 65):
        xs = [0, 1021][:count] + [rng.randrange(1 << 40) for _ in range(max(0, count - 2))]
        first = 3 * count
        rs = X.scalars(SEED, 9, first, count, eng.n)
        want = eng.encrypt(xs, rs).tobytes()
        assert eng.encrypt_seeded(xs, SEED, 9, first).tobytes() == want, (name, count, "host")
        x_len = 8
        xd = torch.frombuffer(bytearray(b"".join(x.to_bytes(x_len, "big") for x in xs)), dtype=torch.uint8).cuda()
        out = torch.zeros(count * E, dtype=torch.uint8, device="cuda")
        eng.encrypt_seeded_dev(xd, x_len, out, count, SEED, 9, first)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want, (name, count, "dev")
        # the rows the caller would hand to a blinded `_dev` call: the same bytes as the oracle's
        rd = torch.zeros(count * nl, dtype=torch.uint8, device="cuda")
        eng.random_scalars_dev(rd, count, SEED, 9, first)
        out2 = torch.zeros(count * E, dtype=torch.uint8, device="cuda")
        eng.encrypt_dev(xd, x_len, rd, nl, out2, count)
        torch.cuda.synchronize()
        assert out2.cpu().numpy().tobytes() == want, (name, count, "rows")


@pytest.mark.parametrize("name", ["toy64", "k256"])
def test_seeded_encryptions_decrypt_to_the_plaintexts(name):
    fx = load_fixture(name)
    pk, sk = engine_key(fx)
    pk.SetupDecryption(sk)
    rng = random.Random(4)
    xs = [0, 1, fx["msg_space"] - 1] + [rng.randrange(fx["msg_space"]) for _ in range(62)]
    cts, seed = pk.EncryptBatchSeeded(xs)
    assert len(seed) == 32 and len(cts) == 65
    m, st = sk.DecryptBatch(cts, pk)
    assert [int(v) for v in m] == xs and not any(st)
    # negative plaintexts as EncryptBatch takes them
    neg = [-1, -500, 7]
    assert [c.C for c in pk.EncryptBatchSeeded(neg, seed, 3)[0]] == [c.C for c in pk.EncryptBatch(neg, X.scalars(seed, 3, 0, 3, pk.N))]
    # given a seed the call is reproducible, and the rows can be recomputed from it
    again, seed2 = pk.EncryptBatchSeeded(xs, seed, 0, 0)
    assert seed2 == seed and [c.C for c in again] == [c.C for c in cts]
    rs = X.scalars(seed, 0, 0, 65, pk.N)
    assert [c.C for c in pk.EncryptBatch(xs, rs)] == [c.C for c in cts]
    other, _ = pk.EncryptBatchSeeded(xs, seed, 1, 0)                      # another stream id: other blinding
    assert all(a.C != b.C for a, b in zip(other, cts))
    assert pk.EncryptBatchSeeded([])[0] == []


def test_multi_engine_shards_by_index():
    """100 elements over three contexts (34 + 33 + 33): every shard expands its own index range."""
    import bgn_amd
    fx = load_fixture("k256")
    eng = engine_key(fx)[0].engine
    me = bgn_amd.MultiEngine(int(fx["p"], 16), int(fx["n"], 16), fx["l"], bytes.fromhex(fx["P"]), bytes.fromhex(fx["Q"]),
                             True, devices=[0, 0, 0])
    try:
        rng = random.Random(100)
        xs = [rng.randrange(1 << 30) for _ in range(100)]
        first = (1 << 32) - 50
        want = eng.encrypt(xs, X.scalars(SEED, 2, first, 100, eng.n)).tobytes()
        assert eng.encrypt_seeded(xs, SEED, 2, first).tobytes() == want
        assert me.encrypt_seeded(xs, SEED, 2, first).tobytes() == want
    finally:
        me.close()


def test_argument_errors_with_a_context():
    import ctypes
    eng = engine("toy64")
    lib = eng._lib
    buf = ctypes.create_string_buffer(4 * eng.elem_bytes)
    seed = ctypes.create_string_buffer(32)
    assert lib.bgn_random_scalars_batch(eng._h, 1, None, 0, 0, buf) == -1
    assert lib.bgn_random_scalars_batch(eng._h, 1, seed, 0, 0, None) == -1
    assert lib.bgn_random_scalars_batch_dev(eng._h, 1, None, 0, 0, buf, None) == -1
    assert lib.bgn_encrypt_seeded_batch(eng._h, 1, buf, 0, seed, 0, 0, buf) == -1
    assert lib.bgn_encrypt_seeded_batch(eng._h, 1, None, 8, seed, 0, 0, buf) == -1
    assert lib.bgn_encrypt_seeded_batch_dev(eng._h, 1, buf, 8, seed, 0, 0, None, None) == -1
    assert lib.bgn_encrypt_seeded_batch(eng._h, 2, buf, 8, seed, 0, (1 << 64) - 1, buf) == -1
    assert lib.bgn_random_scalars_batch(eng._h, 0, None, 0, 0, None) == 0
    assert lib.bgn_encrypt_seeded_batch(eng._h, 0, None, 8, None, 0, 0, None) == 0
    assert buf.raw == bytes(len(buf.raw))
    with pytest.raises(ValueError):
        eng.random_scalars(1, b"short")
