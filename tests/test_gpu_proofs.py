"""GPU: proofs of plaintext knowledge as batch calls with the hash on the device (gadgets.go:32-96) —
bgn_challenge_batch, bgn_prove_plaintext_knowledge_batch, bgn_verify_plaintext_knowledge_batch and their `_dev` twins
against the oracle (oracle/bgn_ref.py) and hashlib.

Keys come from R.NewKeyGen(bits, 1021, 3, True, seed); the fixture keys give 4L mod 64 = 4, 8 and 36 only, so the
padding edges of sha256 bring their own: (224, 1) L = 29, 4L mod 64 = 52 (the padding fits the last block), (232, 1)
L = 30 -> 56 and (232, 2) L = 31 -> 60 (it spills into an extra block).  The 1024-bit key is seed 1: its p has 1031
bits, so L = 129 and an element is 2 mod 4 bytes long.  Proofs of the four Prove keys are recorded in
tests/golden/proofs.json (tests/golden/make_proof_fixtures.py: the oracle's NewProofOfPlaintextKnowledge, each accepted
by its CheckProofOfPlaintextKnoewledge — 40 s of pure Python at 1024 bits, paid once); the oracle also runs live on
the first rows of every key."""
import ctypes
import hashlib
import json
import os
import random

import pytest

import bgn_ref as R
from conftest import GOLDEN, engine_key, load_fixture
from test_gadgets import make_cases

pytestmark = pytest.mark.gpu

GB = 1 << 30
SEEDS = {"k224": (224, 1), "k232a": (232, 1), "k232b": (232, 2), "k128s": (128, 133), "k232s": (232, 1), "k512s": (512, 517),
         "k1024s": (1024, 1)}
_KEYS = {}


def key(name):
    """(oracle pk, oracle sk, engine PublicKey, engine SecretKey) of a seeded key, made once per session."""
    import bgn_amd
    if name not in _KEYS:
        bits, seed = SEEDS[name]
        opk, osk = R.NewKeyGen(bits, 1021, 3, True, seed)
        p = opk.p
        pk = bgn_amd.PublicKey(p, opk.n, opk.l, R.elem_to_bytes(opk.P, p), R.elem_to_bytes(opk.Q, p), 1021)
        if bits >= 1024:
            pk.engine.set_memory_budget(1 * GB)      # small window tables: the key is used for a few hundred encryptions
        _KEYS[name] = (opk, osk, pk, bgn_amd.SecretKey(osk.Key, osk.R))
    return _KEYS[name]


def sha(a: bytes, b: bytes) -> bytes:
    return hashlib.sha256(a + b).digest()


# ---- challenge -----------------------------------------------------------------------------------------------------
def _elements(name, count):
    """(engine, count ciphertexts, count other ciphertexts) of a key: golden ones for the fixture keys, fresh
    encryptions for the seeded ones, repeated in a shuffled order up to `count`."""
    rng = random.Random(count)
    if name in ("k512", "k1024"):
        fx = load_fixture(name)
        eng = engine_key(fx)[0].engine
        pool = [bytes.fromhex(e["ct"]) for e in fx["encrypt"]]
    else:
        eng = key(name)[2].engine
        pool = [bytes(r) for r in eng.encrypt([rng.randrange(1 << 60) for _ in range(24)], [rng.randrange(1 << 60) for _ in range(24)])]
    pick = lambda: [pool[rng.randrange(len(pool))] for _ in range(count)]
    return eng, pick(), pick()


@pytest.mark.parametrize("name,L", [("k224", 29), ("k232a", 30), ("k232b", 31), ("k512", 66), ("k1024", 129)])
def test_challenge_equals_hashlib_on_host_and_device_arrays_at_every_alignment(name, L):
    import torch
    for count in (1, 63, 65, 257):
        eng, a, b = _elements(name, count)
        assert eng.L == L
        want = b"".join(sha(x, y) for x, y in zip(a, b))
        A, B = b"".join(a), b"".join(b)
        assert eng.challenge(A, B).tobytes() == want, (name, count, "host")
        n = len(A)
        for oa, ob in ((0, 0), (1, 2), (2, 3), (3, 1), (0, 3), (2, 0)) if count != 65 else [(i, j) for i in range(4) for j in range(4)]:
            bufa = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
            bufb = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
            bufa[oa:oa + n] = torch.frombuffer(bytearray(A), dtype=torch.uint8).cuda()
            bufb[ob:ob + n] = torch.frombuffer(bytearray(B), dtype=torch.uint8).cuda()
            out = torch.zeros(count * 32 + 4, dtype=torch.uint8, device="cuda")
            oo = (oa + ob) & 3                       # the digests, too, at every alignment
            eng.challenge_dev(bufa[oa:oa + n], bufb[ob:ob + n], out[oo:oo + count * 32], count)
            torch.cuda.synchronize()
            got = out.cpu().numpy().tobytes()
            assert got[oo:oo + count * 32] == want, (name, count, oa, ob)
            assert got[:oo] == bytes(oo) and got[oo + count * 32:] == bytes(4 - oo)      # nothing written outside


def test_challenge_kernel_uses_no_scratch_memory():
    """The message schedule and the state stay in registers: every index is a compile-time constant."""
    fx = load_fixture("k1024")
    eng = engine_key(fx)[0].engine
    cts = b"".join(bytes.fromhex(e["ct"]) for e in fx["encrypt"][:4])
    eng.challenge(cts, cts)
    assert eng.last_kernel_name() == "k_challenge"
    res = (ctypes.c_int64 * 4)()
    assert eng._lib.bgn_last_kernel_resources(eng._h, res) == 0
    vgprs, scratch, lds, threads = list(res)
    assert eng.L == 129 and scratch == 0 and lds == 0 and 0 < vgprs <= 128 and threads >= 256, list(res)


# ---- prove -----------------------------------------------------------------------------------------------------------
with open(os.path.join(GOLDEN, "proofs.json")) as _f:
    RECORDED = json.load(_f)


@pytest.mark.parametrize("name", ["k128s", "k232s", "k512s", "k1024s"])
def test_prove_equals_the_oracle_and_every_proof_verifies(name):
    import bgn_amd
    import torch
    opk, osk, pk, sk = key(name)
    rec = RECORDED[name]
    assert (rec["bits"], rec["seed"]) == SEEDS[name] and int(rec["p"], 16) == opk.p and int(rec["n"], 16) == opk.n
    if name == "k1024s":
        assert opk.p.bit_length() <= 1032 and pk.engine.L == 129        # 2L = 2 mod 4
    p, n, rows = opk.p, opk.n, rec["proofs"]
    assert len(rows) == 70
    vs, zs, ns = ([int(r[k], 16) for r in rows] for k in ("v", "z", "nonce1"))
    assert vs[0] == 0 and zs[1] == 0 and ns[2] == 0 and (vs[3], zs[3], ns[3]) == (n - 1,) * 3
    proofs = pk.NewProofOfPlaintextKnowledgeBatch(sk, vs, zs, ns)
    for i, (pr, r) in enumerate(zip(proofs, rows)):
        assert (pr.Ct.C.hex(), pr.Nonce.C.hex(), pr.DL) == (r["ct"], r["nonce"], int(r["dl"], 16)), (name, i)
    # the oracle live on the first rows: same proof, and it accepts the engine's
    W = lambda c: R.Ciphertext(R.elem_from_bytes(c.C, p) if any(c.C) else None, False)      # (zero bytes: the identity)
    for i in range(4 if name != "k1024s" else 2):
        ref = R.NewProofOfPlaintextKnowledge(opk, osk, vs[i], zs[i], ns[i])
        mine = proofs[i]
        assert (mine.Ct.C, mine.Nonce.C, mine.DL) == (R.elem_to_bytes(ref.Ct.C, p), R.elem_to_bytes(ref.Nonce.C, p), ref.DL)
        assert R.CheckProofOfPlaintextKnoewledge(opk, W(mine.Ct), R.ProofOfPlaintextKnowledge(W(mine.Ct), W(mine.Nonce), mine.DL))
    assert pk.CheckProofOfPlaintextKnoewledgeBatch([pr.Ct for pr in proofs], proofs) == [True] * 70
    # device arrays: the same bytes, nothing downloaded in between; then Verify on the device-resident proofs
    eng = pk.engine
    nl = eng.n_len
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    pack = lambda xs: dev(b"".join(x.to_bytes(nl, "big") for x in xs))
    rq = sk.R * (n // sk.Key) % n
    ct, nonce = (torch.zeros(70 * eng.elem_bytes, dtype=torch.uint8, device="cuda") for _ in range(2))
    dl = torch.zeros(70 * nl, dtype=torch.uint8, device="cuda")
    eng.prove_plaintext_knowledge_dev(pack(vs), nl, pack(zs), nl, pack(ns), nl, pack([rq]), nl, ct, nonce, dl, 70)
    assert eng.last_kernel_name() == "k_pok_response"
    ok = torch.zeros(70, dtype=torch.uint8, device="cuda")
    eng.verify_plaintext_knowledge_dev(ct, ct, nonce, dl, nl, ok, 70)
    torch.cuda.synchronize()
    assert ct.cpu().numpy().tobytes() == b"".join(pr.Ct.C for pr in proofs)
    assert nonce.cpu().numpy().tobytes() == b"".join(pr.Nonce.C for pr in proofs)
    assert dl.cpu().numpy().tobytes() == b"".join(pr.DL.to_bytes(nl, "big") for pr in proofs)
    assert ok.cpu().tolist() == [1] * 70


# ---- verify ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,count", [(128, 12), (512, 6)])
def test_verify_equals_the_oracle_and_the_check_fed_with_host_challenges(bits, count):
    import bgn_amd
    import numpy as np
    import torch
    opk, osk, pk, sk = key("k128s" if bits == 128 else "k512s")
    p, E = opk.p, pk.engine.elem_bytes
    rng = random.Random(bits)
    cases = [(ct, pr) for ct, pr, _ in make_cases(opk, osk, rng, count)]      # valid / wrong randomness / wrong value
    # a proof whose own Ct differs from the ciphertext under test (a valid proof of ANOTHER ciphertext)
    v, z = rng.randrange(opk.n), rng.randrange(opk.n)
    cases.append((cases[0][0], R.NewProofOfPlaintextKnowledge(opk, osk, v, z, rng.randrange(opk.n))))
    # one flipped byte in Nonce (still a well-formed element: the negated point), one flipped byte in DL
    good_ct, good = cases[0]
    x, y = good.Nonce.C
    cases.append((good_ct, R.ProofOfPlaintextKnowledge(good.Ct, R.Ciphertext((x, p - y), False), good.DL)))
    cases.append((good_ct, R.ProofOfPlaintextKnowledge(good.Ct, good.Nonce, good.DL ^ 0x100)))
    want = [R.CheckProofOfPlaintextKnoewledge(opk, ct, pr) for ct, pr in cases]
    assert want[:3] == [True, False, False] and want[count:] == [False, False, False]
    B = lambda c: R.elem_to_bytes(c.C, p)
    cts = b"".join(B(ct) for ct, _ in cases)
    pcs = b"".join(B(pr.Ct) for _, pr in cases)
    nns = bytearray(b"".join(B(pr.Nonce) for _, pr in cases))
    dls = [pr.DL for _, pr in cases]
    eng = pk.engine
    assert eng.verify_plaintext_knowledge(cts, pcs, bytes(nns), dls).tolist() == [int(w) for w in want]
    # a raw byte flip in the Nonce of a valid proof (any byte: the hash changes, and so does the point)
    nns2 = bytearray(nns)
    nns2[E - 1] ^= 1
    got = eng.verify_plaintext_knowledge(cts, pcs, bytes(nns2), dls).tolist()
    flipped = R.ProofOfPlaintextKnowledge(good.Ct, R.Ciphertext(R.elem_from_bytes(bytes(nns2[:E]), p), False), good.DL)
    assert got[0] == int(R.CheckProofOfPlaintextKnoewledge(opk, good_ct, flipped)) == 0
    assert got[1:] == [int(w) for w in want[1:]]
    # the mirror, and the old check fed with hashlib challenges
    W = lambda c: bgn_amd.Ciphertext(B(c), False)
    proofs = [bgn_amd.ProofOfPlaintextKnowledge(W(pr.Ct), W(pr.Nonce), pr.DL) for _, pr in cases]
    assert pk.CheckProofOfPlaintextKnoewledgeBatch([W(ct) for ct, _ in cases], proofs) == want
    N = len(cases)
    c = np.frombuffer(b"".join(sha(pcs[i * E:(i + 1) * E], bytes(nns[i * E:(i + 1) * E])) for i in range(N)), dtype=np.uint8)
    dl = np.frombuffer(b"".join(d.to_bytes(eng.n_len, "big") for d in dls), dtype=np.uint8)
    a, nn = (np.frombuffer(bytes(b), dtype=np.uint8) for b in (cts, nns))
    ok = np.zeros(N, dtype=np.uint8)
    ptr = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    assert eng._lib.bgn_check_plaintext_knowledge_batch(eng._h, N, ptr(a), ptr(nn), ptr(c), 32, ptr(dl), eng.n_len, ptr(ok)) == 0
    assert ok.tolist() == [int(w) for w in want]
    # device arrays
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    okd = torch.zeros(N, dtype=torch.uint8, device="cuda")
    eng.verify_plaintext_knowledge_dev(dev(cts), dev(pcs), dev(nns), dev(dl.tobytes()), eng.n_len, okd, N)
    torch.cuda.synchronize()
    assert okd.cpu().tolist() == [int(w) for w in want]


# ---- mirror ----------------------------------------------------------------------------------------------------------
def test_batch_of_five_equals_five_single_calls_and_drawn_nonces_verify():
    opk, osk, pk, sk = key("k128s")
    rng = random.Random(5)
    n = opk.n
    vs, zs, ns = ([rng.randrange(n) for _ in range(5)] for _ in range(3))
    batch = pk.NewProofOfPlaintextKnowledgeBatch(sk, vs, zs, ns)
    single = [pk.NewProofOfPlaintextKnowledge(sk, v, z, a) for v, z, a in zip(vs, zs, ns)]
    assert [(b.Ct.C, b.Nonce.C, b.DL) for b in batch] == [(s.Ct.C, s.Nonce.C, s.DL) for s in single]
    drawn = pk.NewProofOfPlaintextKnowledgeBatch(sk, vs, zs)                  # nonces from `secrets`
    assert [d.Ct.C for d in drawn] == [b.Ct.C for b in batch] and all(0 <= d.DL < n for d in drawn)
    assert pk.CheckProofOfPlaintextKnoewledgeBatch([d.Ct for d in drawn], drawn) == [True] * 5
    assert pk.NewProofOfPlaintextKnowledgeBatch(sk, [], []) == []


def test_argument_errors_are_reported_before_any_work():
    opk, osk, pk, sk = key("k128s")
    eng, lib = pk.engine, pk.engine._lib
    nl, E = eng.n_len, eng.elem_bytes
    buf = ctypes.create_string_buffer(4 * E)
    big = ctypes.create_string_buffer(nl + 1)
    args = lambda **kw: [kw.get(k, d) for k, d in (("v", buf), ("vl", nl), ("z", buf), ("zl", nl), ("a", buf), ("al", nl),
                                                   ("rq", buf), ("rl", nl), ("ct", buf), ("nn", buf), ("dl", buf))]
    for bad in (dict(vl=nl + 1, v=big), dict(zl=nl + 1), dict(al=nl + 1), dict(rl=nl + 1), dict(rl=0), dict(vl=0), dict(v=None),
                dict(rq=None), dict(dl=None)):
        assert lib.bgn_prove_plaintext_knowledge_batch(eng._h, 1, *args(**bad)) == -1, bad
        assert lib.bgn_prove_plaintext_knowledge_batch_dev(eng._h, 1, *args(**bad), None) == -1, bad
    assert lib.bgn_challenge_batch(eng._h, 1, buf, None, buf) == -1
    assert lib.bgn_verify_plaintext_knowledge_batch(eng._h, 1, buf, buf, buf, buf, 0, buf) == -1
    assert lib.bgn_verify_plaintext_knowledge_batch(eng._h, 1, buf, None, buf, buf, nl, buf) == -1
