"""Regenerates tests/golden/proofs.json: proofs of plaintext knowledge computed by the oracle (oracle/bgn_ref.py
NewProofOfPlaintextKnowledge) for fixed inputs, each checked by the oracle's CheckProofOfPlaintextKnoewledge before it
is recorded.  TEST INFRASTRUCTURE: tests/test_gpu_proofs.py compares the engine's proofs with these byte for byte
(70 proofs of a 1024-bit key take the pure-Python oracle 40 s; recorded once they cost the suite nothing) and runs the
oracle live on a few rows of every key.

    python tests/golden/make_proof_fixtures.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bgn_ref as R  # noqa: E402

# name -> (key bits, seed) of R.NewKeyGen(bits, 1021, 3, True, seed); k1024s: p has 1031 bits, so L = 129 and 2L = 2 mod 4
KEYS = {"k128s": (128, 133), "k232s": (232, 1), "k512s": (512, 517), "k1024s": (1024, 1)}
COUNT = 70


def rows(n: int, seed: int):
    """(v, z, nonce1) triples: the edge rows first (v = 0, z = 0, nonce1 = 0, everything n - 1), then plaintext-sized
    and full-size values."""
    rng = random.Random(seed)
    r = lambda: rng.randrange(n)
    out = [(0, r(), r()), (r(), 0, r()), (r(), r(), 0), (n - 1, n - 1, n - 1), (1, 1, 1), (0, r(), 0)]
    while len(out) < COUNT:
        out.append((rng.randrange(1021) if len(out) % 2 else r(), r(), r()))
    return out


def main():
    doc = {}
    for name, (bits, seed) in KEYS.items():
        pk, sk = R.NewKeyGen(bits, 1021, 3, True, seed)
        p = pk.p
        recs = []
        for v, z, a in rows(pk.n, seed):
            pr = R.NewProofOfPlaintextKnowledge(pk, sk, v, z, a)
            assert R.CheckProofOfPlaintextKnoewledge(pk, pk.EncryptWithRandomness(v, z), pr)
            recs.append({"v": hex(v), "z": hex(z), "nonce1": hex(a), "ct": R.elem_to_bytes(pr.Ct.C, p).hex(),
                         "nonce": R.elem_to_bytes(pr.Nonce.C, p).hex(), "dl": hex(pr.DL)})
        doc[name] = {"bits": bits, "seed": seed, "p": hex(p), "n": hex(pk.n), "proofs": recs}
        print(name, "L =", (p.bit_length() + 7) // 8, len(recs), "proofs")
    with open(os.path.join(HERE, "proofs.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
