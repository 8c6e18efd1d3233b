"""GPU: the golden vectors of the 37-limb key (tests/golden/k1024b.json) beyond Add, Sub and Neg: Encrypt, Mult on each
of the three kernel families, makeL2, MultConst and Decrypt on both levels, the polynomial product.  k1024b is the one
fixture key whose limb count is not a multiple of four below the top (10 limbs per lane, the top limb at index 6 of
lane 3) and, as p = 2 mod 3, the one production-size key whose Mult keeps the Miller loop on the curve a = 1.
conftest.KEYS stops at k1024, so the parametrised golden tests of test_gpu_parity.py never reach it.  The key has an
engine and a memory budget of its own (as in test_gpu_quad.py), made once for the module."""
import pytest

from conftest import load_fixture

pytestmark = pytest.mark.gpu

NAME = "k1024b"


def H(hexes):
    return b"".join(bytes.fromhex(h) for h in hexes)


@pytest.fixture(scope="module")
def key():
    import bgn_amd
    fx = load_fixture(NAME)
    pk = bgn_amd.PublicKey(int(fx["p"], 16), int(fx["n"], 16), fx["l"], bytes.fromhex(fx["P"]), bytes.fromhex(fx["Q"]),
                           fx["msg_space"], True, fx["poly_base"])
    sk = bgn_amd.SecretKey(int(fx["q1"], 16))
    pk.engine.set_memory_budget(40 << 30)
    assert pk.engine.L == fx["fp_bytes"]
    yield fx, pk, sk
    pk.engine.close()


def test_encrypt_golden(key, engopts):
    fx, pk, _ = key
    eng = engopts.register(pk.engine)
    out = eng.encrypt([int(e["x"], 16) for e in fx["encrypt"]], [int(e["r"], 16) for e in fx["encrypt"]])
    for row, e in zip(out, fx["encrypt"]):
        assert bytes(row).hex() == e["ct"], "Encrypt(x=%s, r=%s)" % (e["x"], e["r"])


@pytest.mark.parametrize("kernel", ["coop", "quad", "lane"])
def test_mult_golden_on_each_family(key, kernel, engopts):
    fx, pk, _ = key
    eng = engopts.register(pk.engine)
    engopts.force(kernel)
    cts = [e["ct"] for e in fx["encrypt"]]
    out = eng.mult(H([cts[v["a"]] for v in fx["mult"]]), H([cts[v["b"]] for v in fx["mult"]]))
    name = eng.last_kernel_name()
    assert ("coop" in name, "quad" in name) == (kernel == "coop", kernel == "quad"), name
    for row, v in zip(out, fx["mult"]):
        assert bytes(row).hex() == v["out"], "Mult(%d, %d) on %s" % (v["a"], v["b"], name)


def test_make_l2_golden(key, engopts):
    fx, pk, _ = key
    eng = engopts.register(pk.engine)
    cts = [e["ct"] for e in fx["encrypt"]]
    out = eng.make_l2(H([cts[v["a"]] for v in fx["make_l2"]]))
    for row, v in zip(out, fx["make_l2"]):
        assert bytes(row).hex() == v["out"], "makeL2(%d)" % v["a"]


def test_multconst_golden_on_both_levels(key, engopts):
    fx, pk, _ = key
    eng = engopts.register(pk.engine)
    cts = [e["ct"] for e in fx["encrypt"]]
    l2 = [v["out"] for v in fx["mult"]]
    for lvl, rows, src in ((1, fx["multconst_l1"], cts), (2, fx["multconst_l2"], l2)):
        out = eng.multconst(lvl, H([src[v["a"]] for v in rows]), [int(v["k"], 16) for v in rows])
        for row, v in zip(out, rows):
            assert bytes(row).hex() == v["out"], "MultConst L%d(%d, k=%s)" % (lvl, v["a"], v["k"])


def test_decrypt_golden_on_both_levels(key, engopts):
    fx, pk, sk = key
    eng = engopts.register(pk.engine)
    pk.SetupDecryption(sk)
    for lvl in (1, 2):
        items = [d for d in fx["decrypt"] if d["level"] == lvl]
        assert items
        m, st = eng.decrypt(lvl, H([d["ct"] for d in items]))
        for d, mi, si in zip(items, m, st):
            if d["expect"] is None:
                assert si == 1, "L%d: m=%s must be out of bounds" % (lvl, d["m"])
            else:
                assert si == 0 and int(mi) == d["expect"], "L%d: Decrypt(m=%s) -> %d, status %d" % (lvl, d["m"], mi, si)


def test_poly_mult_golden(key, engopts):
    fx, pk, _ = key
    eng = engopts.register(pk.engine)
    po = fx["poly"]
    out = eng.poly_mult(1, po["d1"], po["d2"], H(po["a"]), H(po["b"]))
    assert [bytes(r).hex() for r in out] == po["out"]
