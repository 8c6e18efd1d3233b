"""Rates of the proof entry points on one GPU (profiles/r08_proof_rates.csv), 1024-bit key, device-resident arrays,
one process, five runs each: median and max - min.

  (a) Verify: bgn_verify_plaintext_knowledge_batch_dev (challenge on the device) against the route a caller had before
      it — download Ct and Nonce, one hashlib call per proof, upload the digests, bgn_check_plaintext_knowledge_batch_dev
      — on the same arrays.
  (b) Prove: bgn_prove_plaintext_knowledge_batch_dev against the one-proof-at-a-time host routine it replaces (an
      EncryptBatch of two elements, hashlib and Python integers per proof), timed on 256 proofs and SCALED to the batch.
  (c) The two new kernels by HIP events (bgn_last_kernel_ms): what share of the chain the challenge is.

    python tools/proof_rates.py [--log2 16 20] [--out profiles/r08_proof_rates.csv]
"""
import argparse
import csv
import hashlib
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RUNS = 5


def timed(fn, sync):
    out = []
    for _ in range(RUNS):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), max(out) - min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_proof_rates.csv"))
    args = ap.parse_args()
    import torch
    import bgn_amd
    import bgn_ref as R
    opk, osk = R.NewKeyGen(1024, 1021, 3, True, 1)                      # p of 1031 bits: L = 129
    p, n = opk.p, opk.n
    pk = bgn_amd.PublicKey(p, n, opk.l, R.elem_to_bytes(opk.P, p), R.elem_to_bytes(opk.Q, p), 1021)
    sk = bgn_amd.SecretKey(osk.Key, osk.R)
    eng = pk.engine
    E, nl = eng.elem_bytes, eng.n_len
    rq = sk.R * (n // sk.Key) % n
    sync = torch.cuda.synchronize
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    rows = []

    def record(what, count, med, spread, note=""):
        rows.append([what, count, RUNS, "%.3f" % med, "%.3f" % spread, "%.4g" % (count / med * 1e3), note])
        print(rows[-1], flush=True)

    rng = random.Random(8)
    for lg in args.log2:
        N = 1 << lg
        v, z, a = (dev(rng.randbytes(N * nl)) for _ in range(3))          # any value that fits is taken (values >= n too)
        k = dev(rq.to_bytes(nl, "big"))
        ct, nonce = (torch.zeros(N * E, dtype=torch.uint8, device="cuda") for _ in range(2))
        dl = torch.zeros(N * nl, dtype=torch.uint8, device="cuda")
        ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
        c = torch.zeros(N * 32, dtype=torch.uint8, device="cuda")
        prove = lambda: eng.prove_plaintext_knowledge_dev(v, nl, z, nl, a, nl, k, nl, ct, nonce, dl, N)
        prove()                                                           # warm-up: window tables, workspace
        sync()
        record("prove_dev", N, *timed(prove, sync))
        record("k_pok_response (HIP events)", N, eng.last_kernel_ms(), 0.0, eng.last_kernel_name())

        # (b) the host routine this replaces, on a sample
        S = 256
        vs, zs, ns = ([rng.randrange(n) for _ in range(S)] for _ in range(3))

        def parent_prove():
            for x, r, a1 in zip(vs, zs, ns):
                c1, c2 = pk.EncryptBatch([x, a1], [r, 0])
                h = int.from_bytes(hashlib.sha256(c1.C + c2.C).digest(), "big")
                _ = (a1 + h * x + sk.R * r * h * (n // sk.Key)) % n
        med, spread = timed(parent_prove, sync)
        record("prove_parent_loop", N, med * N / S, spread * N / S, "SCALED from %d proofs (%.1f ms)" % (S, med))

        # (a) verify, both routes on the same device arrays
        verify = lambda: eng.verify_plaintext_knowledge_dev(ct, ct, nonce, dl, nl, ok, N)
        verify()
        sync()
        assert int(ok.sum().item()) == N, "the proofs just made must verify"
        record("verify_dev", N, *timed(verify, sync))
        parts = {}

        def parent_verify():
            t0 = time.perf_counter()
            hc, hn = ct.cpu().numpy().tobytes(), nonce.cpu().numpy().tobytes()
            t1 = time.perf_counter()
            dig = b"".join(hashlib.sha256(hc[i * E:(i + 1) * E] + hn[i * E:(i + 1) * E]).digest() for i in range(N))
            t2 = time.perf_counter()
            c.copy_(torch.frombuffer(bytearray(dig), dtype=torch.uint8))
            sync()
            t3 = time.perf_counter()
            bgn_amd._lib.check(eng._lib.bgn_check_plaintext_knowledge_batch_dev(eng._h, N, ct.data_ptr(), nonce.data_ptr(), c.data_ptr(),
                                                                                32, dl.data_ptr(), nl, ok.data_ptr(), None),
                               "bgn_check_plaintext_knowledge_batch_dev")
            sync()
            t4 = time.perf_counter()
            parts["download"], parts["hashlib"], parts["upload"], parts["check_dev"] = ((y - x) * 1e3 for x, y in
                                                                                       ((t0, t1), (t1, t2), (t2, t3), (t3, t4)))
        med, spread = timed(parent_verify, sync)
        assert int(ok.sum().item()) == N
        record("verify_parent_route", N, med, spread, "last run: " + " ".join("%s %.1f ms" % kv for kv in parts.items()))
        ch = lambda: eng.challenge_dev(ct, nonce, c, N)
        ch()
        ms = []
        for _ in range(RUNS):
            ch()
            ms.append(eng.last_kernel_ms())
        record("k_challenge (HIP events)", N, statistics.median(ms), max(ms) - min(ms), eng.last_kernel_name())
        del v, z, a, ct, nonce, dl, ok, c
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["what", "count", "runs", "median_ms", "max_minus_min_ms", "per_second", "note"])
        w.writerows(rows)


if __name__ == "__main__":
    main()
