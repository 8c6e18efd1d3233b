"""GPU: Mult's lane kernel with its Miller loop on the isomorphic curve y^2 = x^3 - 3x (option miller_a3, default on;
pairing.hpp miller_double) gives the bytes of the loop on y^2 = x^3 + x (miller_a3 = 0), of the golden vectors and of
the C oracle — one pairing per lane and runs of three with a ragged tail, the width-5 loop and the plain NAF, at 10, 19
and 36 limbs — and is inactive for a key whose field has no fourth root of -3."""
import random

import pytest

from conftest import engine_key, load_fixture

pytestmark = pytest.mark.gpu


def H(hexes):
    return b"".join(bytes.fromhex(h) for h in hexes)


def lane_only(engopts):
    engopts.set("quad_min", 0)
    engopts.set("quad_max", 0)
    engopts.set("coop_max", 0)


def make_engine(fx, monkeypatch, window):
    """A context of its own whose general Miller loop runs over the plain NAF (miller_window is read at creation)."""
    import bgn_amd
    monkeypatch.setenv("BGN_MILLER_WINDOW", str(window))
    pk = bgn_amd.PublicKey(int(fx["p"], 16), int(fx["n"], 16), fx["l"], bytes.fromhex(fx["P"]), bytes.fromhex(fx["Q"]),
                           fx["msg_space"], True, fx["poly_base"])
    monkeypatch.delenv("BGN_MILLER_WINDOW")
    return pk.engine


_CASES = {}


def operands(name):
    """(a, b, expected) for one key, built once: the golden pairs, random pairs checked by the C oracle, an identity on
    either side, A = B, B = -A, an operand off the curve and the zero-norm pair; 263 pairs (two workgroups with one
    pairing per lane, a ragged last run with three)."""
    if name in _CASES:
        return _CASES[name]
    import oracle_c
    fx = load_fixture(name)
    pk, _ = engine_key(fx)
    eng = pk.engine
    E, L = eng.elem_bytes, eng.elem_bytes // 2
    p, n = int(fx["p"], 16), int(fx["n"], 16)
    cts = [bytes.fromhex(e["ct"]) for e in fx["encrypt"]]
    ga, gb = [cts[v["a"]] for v in fx["mult"]], [cts[v["b"]] for v in fx["mult"]]
    want = [bytes.fromhex(v["out"]) for v in fx["mult"]]
    rng = random.Random(2718)
    nr = 10
    fresh = eng.encrypt([rng.randrange(fx["msg_space"]) for _ in range(2 * nr)], [rng.randrange(n) for _ in range(2 * nr)])
    fresh = [bytes(r) for r in fresh]
    ra, rb = fresh[:nr], fresh[nr:]
    neg = lambda c: c[:L] + ((p - int.from_bytes(c[L:], "big")) % p).to_bytes(L, "big")
    zero = bytes(E)
    ra += [zero, fresh[0], fresh[1], fresh[2]]
    rb += [fresh[1], zero, fresh[1], neg(fresh[2])]               # identity | identity | A = B | B = -A
    o = oracle_c.Oracle.from_fixture(fx)
    ow = o.mult(b"".join(ra), b"".join(rb))
    want += [ow[i * E:(i + 1) * E] for i in range(len(ra))]
    one = (1).to_bytes(L, "big") + bytes(L)
    assert want[len(ga) + nr] == one and want[len(ga) + nr + 1] == one
    a, b = ga + ra, gb + rb
    # not on the curve: a flipped low bit of y (no reference value: only a = -3 against a = 1), and the pair whose
    # tangent vanishes at phi(B), N(f) = 0: the identity (tests/test_gpu_quad.py)
    off = fresh[3][:E - 1] + bytes([fresh[3][E - 1] ^ 1])
    a += [off, fresh[4], (5).to_bytes(L, "big") + bytes(L)]
    b += [fresh[5], off, (p - 5).to_bytes(L, "big") + (7).to_bytes(L, "big")]
    want += [None, None, one]
    k = 0
    while len(a) < 263:                                           # fill with the random pairs again
        a.append(ra[k % nr])
        b.append(rb[k % nr])
        want.append(want[len(ga) + k % nr])
        k += 1
    _CASES[name] = (b"".join(a), b"".join(b), want)
    return _CASES[name]


@pytest.mark.parametrize("window", [5, 0])
@pytest.mark.parametrize("name,nl", [("k256", 10), ("k512", 19), ("k1024", 36)])
def test_mult_on_the_a3_curve_equals_the_a1_path(name, nl, window, engopts, monkeypatch):
    fx = load_fixture(name)
    a, b, want = operands(name)
    if window == 5:
        eng = engine_key(fx)[0].engine
    else:
        eng = engopts.register(make_engine(fx, monkeypatch, window))
    lane_only(engopts)
    assert eng.get_option("miller_window") == window
    E = eng.elem_bytes
    got = {}
    for run in (1, 3):
        engopts.set("pairing_run", run)
        for a3 in (0, 1):
            engopts.set("miller_a3", a3)
            assert eng.get_option("miller_a3") == a3              # p = 1 mod 3: the route is active when asked for
            got[run, a3] = eng.mult(a, b).tobytes()
            assert eng.last_kernel_name() == "k_pairing<%d, 0>" % nl
    assert got[1, 1] == got[1, 0], "one pairing per lane: a = -3 differs from a = 1"
    assert got[3, 1] == got[3, 0], "runs of three: a = -3 differs from a = 1"
    assert got[3, 1] == got[1, 1]
    for i, w in enumerate(want):
        if w is not None:
            assert got[1, 1][i * E:(i + 1) * E] == w, "pair %d against the golden / oracle bytes" % i


def test_default_is_on_and_a_key_without_the_root_stays_on_a1(engopts, monkeypatch):
    """The option defaults to 1.  k1024b (p = 2 mod 3, 37 limbs) has no fourth root of -3: the option reads back 0
    whatever is set, and Mult gives the golden bytes either way on the same kernel."""
    fx = load_fixture("k256")
    eng = engine_key(fx)[0].engine
    assert eng.get_option("miller_a3") == 1
    fx = load_fixture("k1024b")
    assert int(fx["p"], 16) % 3 != 1
    eng = engopts.register(make_engine(fx, monkeypatch, 5))
    lane_only(engopts)
    cts = [e["ct"] for e in fx["encrypt"]]
    rows = fx["mult"][:6]
    a, b = H([cts[v["a"]] for v in rows]), H([cts[v["b"]] for v in rows])
    for a3 in (1, 0):
        engopts.set("miller_a3", a3)
        assert eng.get_option("miller_a3") == 0
        out = eng.mult(a, b)
        assert eng.last_kernel_name() == "k_pairing<37, 0>"
        for row, v in zip(out, rows):
            assert bytes(row).hex() == v["out"]
