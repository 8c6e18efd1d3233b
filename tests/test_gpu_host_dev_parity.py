"""GPU: every host-buffer entry point returns the bytes of its _dev twin, on each of its routes.

The calls without a suffix stage host arrays through device memory around the _dev entry points (engine.cpp
host_call): through the combiner of concurrent small calls, through the chunked pipeline (Add / Sub / Neg on large
arrays) or with one blocking copy per array.  Each case runs the host call, then bgn_dev_upload -> the _dev call on
the null stream -> bgn_dev_download on the same inputs, and compares the results byte for byte: counts 1 and 65 (65
crosses the 64-element stride padding of the workspaces), the optional randomness present and absent, option
combine = 0 and 1 for the eight combinable calls, and for Add / Sub / Neg the pipeline with a ragged last chunk."""
import functools
import hashlib
import random

import numpy as np
import pytest

from bgn_amd._lib import check
from bgn_amd.api import _ptr, _scalars
from conftest import engine_key, load_fixture

pytestmark = pytest.mark.gpu

N = 100                      # rows of every input pool; the pipeline cases use all of them
BEYOND = 10 ** 6             # a plaintext beyond the discrete-log table of every fixture (B*B+B+2 for T = 1021)


@functools.lru_cache(maxsize=None)
def _pool(name):
    """Inputs of one key, made once: level-1 and level-2 ciphertexts, scalars, randomness."""
    fx = load_fixture(name)
    pk, sk = engine_key(fx)
    pk.SetupDecryption(sk)
    eng = pk.engine
    rng = random.Random(17)
    n, T = int(fx["n"], 16), fx["msg_space"]
    xs = [rng.randrange(T) for _ in range(N)]
    xs[0] = BEYOND
    r_len = (n.bit_length() + 7) // 8
    d = {"xs": xs, "X": _scalars(xs), "R": _scalars([rng.randrange(n) for _ in range(N)], r_len),
         "K": _scalars([rng.randrange(1, 1 << 40) for _ in range(N)], 5)}
    d["R0"] = _scalars([rng.randrange(n) for _ in range(N)], r_len)
    d["A"] = eng.encrypt(xs, [int.from_bytes(bytes(r), "big") for r in d["R0"]])
    d["B"] = eng.encrypt([rng.randrange(T) for _ in range(N)])
    d["A2"], d["B2"] = eng.make_l2(d["A"]), eng.make_l2(d["B"])
    return d


def _eng(name):
    return engine_key(load_fixture(name))[0].engine


def _rows(a, count):
    """`count` rows of a pool array (cyclically, for the polynomial cases that need more than N)."""
    return None if a is None else np.ascontiguousarray(a[np.arange(count) % len(a)])


def _both(eng, name, ins, outs, args):
    """Runs `name` on host arrays and `name`_dev on uploaded copies; asserts equal bytes; returns the host results.
    ins: uint8 arrays (None: an optional array left out); outs: arrays of the results' shapes;
    args(in_ptrs, out_ptrs): the arguments after the context (the _dev twin takes the same, then the stream)."""
    lib, h = eng._lib, eng._h
    host = [np.zeros_like(o) for o in outs]
    check(getattr(lib, name)(h, *args([_ptr(a) for a in ins], [_ptr(o) for o in host])), name)
    dev = [np.full_like(o, 0x5a) for o in outs]
    owned = []

    def alloc(a):
        if a is None:
            return None
        p = lib.bgn_dev_alloc(h, a.nbytes)
        assert p, "bgn_dev_alloc"
        owned.append(p)
        return p

    try:
        din, dout = [alloc(a) for a in ins], [alloc(o) for o in dev]
        for a, p in zip(ins, din):
            if a is not None:
                check(lib.bgn_dev_upload(h, p, _ptr(a), a.nbytes), "bgn_dev_upload")
        check(getattr(lib, name + "_dev")(h, *args(din, dout), None), name + "_dev")
        for o, p in zip(dev, dout):
            check(lib.bgn_dev_download(h, _ptr(o), p, o.nbytes), "bgn_dev_download")
    finally:
        for p in owned:
            lib.bgn_dev_free(h, p)
    for i, (x, y) in enumerate(zip(host, dev)):
        assert x.tobytes() == y.tobytes(), "%s: output %d differs from %s_dev" % (name, i, name)
    return host


def _elems(eng, count):
    return np.zeros((count, eng.elem_bytes), dtype=np.uint8)


def _ct(d, level, which="A"):
    return d[which + ("2" if level == 2 else "")]


# name -> its levels, whether its last input is the optional randomness, inputs(pool, level) and
# args(pool, count, level, r_len) -> the argument builder _both takes
COMBINABLE = {
    "bgn_encrypt_batch": dict(levels=(1,), blind=True, ins=lambda d, lvl: [d["X"], d["R"]],
                              args=lambda d, n, lvl, rl: lambda i, o: (n, i[0], d["X"].shape[1], i[1], rl, o[0])),
    "bgn_add_batch": dict(levels=(1, 2), blind=True, ins=lambda d, lvl: [_ct(d, lvl), _ct(d, lvl, "B"), d["R"]],
                          args=lambda d, n, lvl, rl: lambda i, o: (n, lvl, i[0], i[1], i[2], rl, o[0])),
    "bgn_sub_batch": dict(levels=(1, 2), blind=True, ins=lambda d, lvl: [_ct(d, lvl), _ct(d, lvl, "B"), d["R"]],
                          args=lambda d, n, lvl, rl: lambda i, o: (n, lvl, i[0], i[1], i[2], rl, o[0])),
    "bgn_neg_batch": dict(levels=(1, 2), blind=False, ins=lambda d, lvl: [_ct(d, lvl)],
                          args=lambda d, n, lvl, rl: lambda i, o: (n, lvl, i[0], o[0])),
    "bgn_mult_batch": dict(levels=(1,), blind=True, ins=lambda d, lvl: [d["A"], d["B"], d["R"]],
                           args=lambda d, n, lvl, rl: lambda i, o: (n, i[0], i[1], i[2], rl, o[0])),
    "bgn_make_l2_batch": dict(levels=(1,), blind=False, ins=lambda d, lvl: [d["A"]],
                              args=lambda d, n, lvl, rl: lambda i, o: (n, i[0], o[0])),
    "bgn_multconst_batch": dict(levels=(1, 2), blind=True, ins=lambda d, lvl: [_ct(d, lvl), d["K"], d["R"]],
                                args=lambda d, n, lvl, rl: lambda i, o: (n, lvl, i[0], i[1], d["K"].shape[1], i[2], rl, o[0])),
    "bgn_decrypt_batch": dict(levels=(1, 2), blind=False, ins=lambda d, lvl: [_ct(d, lvl)],
                              args=lambda d, n, lvl, rl: lambda i, o: (n, lvl, i[0], o[0], o[1])),
}


def _combinable_case(eng, d, name, level, count, blinded):
    spec = COMBINABLE[name]
    ins = [_rows(a, count) for a in spec["ins"](d, level)]
    r_len = 0
    if spec["blind"]:
        r_len = ins[-1].shape[1] if blinded else 0
        if not blinded:
            ins[-1] = None
    if name == "bgn_decrypt_batch":
        outs = [np.zeros(count, dtype=np.int64), np.zeros(count, dtype=np.uint8)]
    else:
        outs = [_elems(eng, count)]
    return _both(eng, name, ins, outs, spec["args"](d, count, level, r_len))


@pytest.mark.parametrize("key,name", [("toy64", n) for n in COMBINABLE] +
                         [("k512", "bgn_mult_batch"), ("k512", "bgn_make_l2_batch")])
def test_combinable_call_equals_its_dev_twin_with_and_without_the_combiner(key, name, engopts):
    """Counts 1 and 65, both levels, randomness present and absent; combine = 1: the lone caller is its own leader
    (the combiner's call counter moves by one), combine = 0: one-shot staging (the counter stays)."""
    d, eng = _pool(key), _eng(key)
    spec = COMBINABLE[name]
    engopts.set("host_pipe", 0)
    for combine in (0, 1):
        engopts.set("combine", combine)
        for level in spec["levels"]:
            for count in (1, 65):
                for blinded in ((False, True) if spec["blind"] else (False,)):
                    before = eng.combiner_stats()["calls"]
                    out = _combinable_case(eng, d, name, level, count, blinded)
                    assert eng.combiner_stats()["calls"] - before == combine, (name, level, count, blinded)
                    if name == "bgn_decrypt_batch":
                        m, st = out
                        assert st[0] == 1 and m[0] == 0                     # xs[0] is beyond the table
                        if count > 1:
                            assert not st[1:].any() and m[1:].tolist() == d["xs"][1:count]


@pytest.mark.parametrize("name", ["bgn_add_batch", "bgn_sub_batch", "bgn_neg_batch"])
def test_pipelined_call_equals_its_dev_twin(name, engopts, capfd):
    """100 elements in chunks of 32 (three full chunks and a ragged fourth) over the staging ring, both levels, blinded
    Add / Sub with the optional array in the ring; the same call staged in one shot (host_pipe = 0).  The combiner is
    off: it would take a call of this size before the pipeline is considered.  Option host_pipe_trace pins the route:
    the pipelined call reports its four launches on stderr, the one-shot call reports nothing."""
    d, eng = _pool("toy64"), _eng("toy64")
    spec = COMBINABLE[name]
    engopts.set("combine", 0)
    engopts.set("host_pipe_chunk", 32)
    engopts.set("host_pipe_trace", 1)
    for level in (1, 2):
        for blinded in ((False, True) if spec["blind"] else (False,)):
            engopts.set("host_pipe", 1)
            capfd.readouterr()
            piped = _combinable_case(eng, d, name, level, N, blinded)
            trace = capfd.readouterr().err
            assert [trace.count("[pipe]"), trace.count(" launched ")] == [14, 4], trace   # set up, 3 x 4 chunks, joined
            engopts.set("host_pipe", 0)
            one = _combinable_case(eng, d, name, level, N, blinded)
            assert "[pipe]" not in capfd.readouterr().err
            assert piped[0].tobytes() == one[0].tobytes()


@pytest.mark.parametrize("name", ["bgn_encrypt_batch", "bgn_mult_batch", "bgn_make_l2_batch", "bgn_multconst_batch",
                                  "bgn_decrypt_batch"])
def test_only_add_sub_neg_are_pipelined(name, engopts, capfd):
    """The other combinable calls stage in one shot at the size and options that pipeline Add / Sub / Neg."""
    d, eng = _pool("toy64"), _eng("toy64")
    engopts.set("combine", 0)
    engopts.set("host_pipe", 1)
    engopts.set("host_pipe_chunk", 32)
    engopts.set("host_pipe_trace", 1)
    capfd.readouterr()
    _combinable_case(eng, d, name, 1, N, False)
    assert "[pipe]" not in capfd.readouterr().err


@pytest.mark.parametrize("npoly", [1, 65])
def test_poly_calls_equal_their_dev_twins(npoly):
    d, eng = _pool("toy64"), _eng("toy64")
    d1, d2 = 2, 3
    _both(eng, "bgn_poly_mult_batch", [_rows(d["A"], npoly * d1), _rows(d["B"], npoly * d2)],
          [_elems(eng, npoly * (d1 + d2))], lambda i, o: (npoly, d1, d2, i[0], i[1], o[0]))
    dd, dp, k_len = 3, 2, d["K"].shape[1]
    for level in (1, 2):
        ct = _rows(_ct(d, level), npoly * dd)
        for per_poly in (0, 1):                                             # one scalar row set, or one per polynomial
            k = _rows(d["K"], (npoly if per_poly else 1) * dp)
            _both(eng, "bgn_poly_multconst_batch", [ct, k], [_elems(eng, npoly * (dd + dp))],
                  lambda i, o: (npoly, dd, dp, level, i[0], i[1], k_len, per_poly, o[0]))
        _both(eng, "bgn_poly_eval_batch", [ct], [_elems(eng, npoly)], lambda i, o: (npoly, dd, level, i[0], 3, o[0]))


@pytest.mark.parametrize("count", [1, 65])
def test_validate_and_proof_checks_equal_their_dev_twins(count):
    fx = load_fixture("toy64")
    d, eng = _pool("toy64"), _eng("toy64")
    pk, sk = engine_key(fx)
    ok = np.zeros(count, dtype=np.uint8)
    for level in (1, 2):
        ct = _rows(_ct(d, level), count).copy()
        ct[count // 2] = 0xff                                               # not a field element
        got, = _both(eng, "bgn_validate_batch", [ct], [ok], lambda i, o: (count, level, i[0], o[0]))
        assert got.tolist() == [0 if i == count // 2 else 1 for i in range(count)]
    # DecryptionProof: A = Encrypt(xs, R0); a wrong value in one row
    v = _rows(d["X"], count).copy()
    v[count // 2, -1] ^= 1
    got, = _both(eng, "bgn_check_decryption_proof_batch", [_rows(d["A"], count), v, _rows(d["R0"], count)], [ok],
                 lambda i, o: (count, i[0], i[1], v.shape[1], i[2], d["R0"].shape[1], o[0]))
    assert got.tolist() == [0 if i == count // 2 else 1 for i in range(count)]
    # ProofOfPlaintextKnowledge of deterministic ciphertexts (z = 0): ct^c * nonce == P^DL with DL = nonce1 + c * v;
    # a wrong DL in one row
    n = int(fx["n"], 16)
    rng = random.Random(23)
    vs = [rng.randrange(fx["msg_space"]) for _ in range(count)]
    n1 = [rng.randrange(n) for _ in range(count)]
    ct, nonce = eng.encrypt(vs), eng.encrypt(n1)
    cs = [int.from_bytes(hashlib.sha256(a.tobytes() + b.tobytes()).digest(), "big") for a, b in zip(ct, nonce)]
    dls = [(a + c * x) % n for a, c, x in zip(n1, cs, vs)]
    dls[count // 2] = (dls[count // 2] + 1) % n
    c_be, dl_be = _scalars(cs, 32), _scalars(dls, 8)
    got, = _both(eng, "bgn_check_plaintext_knowledge_batch", [ct, nonce, c_be, dl_be], [ok],
                 lambda i, o: (count, i[0], i[1], i[2], 32, i[3], 8, o[0]))
    assert got.tolist() == [0 if i == count // 2 else 1 for i in range(count)]
