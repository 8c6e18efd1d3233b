"""Rates of the seeded-randomness entry points on one GPU (profiles/r09_seeded_random.csv), 1024-bit key, one process,
five runs each: median and max - min.

  (a) k_random_scalars alone on a device-resident array: wall time of bgn_random_scalars_batch_dev and the kernel by
      HIP events (bgn_last_kernel_ms).
  (b) Blinded Encrypt of host plaintexts by the route a caller had before: host rows from os.urandom(count * n_len) —
      the fastest thing a host can do — then bgn_encrypt_batch(x, r).
  (c) The same by bgn_encrypt_seeded_batch.  (b) and (c) alternate run by run in this process.
  (d) Vector registers, scratch bytes and LDS bytes of k_random_scalars per limb count (bgn_last_kernel_resources), on
      the fixture keys.

    python tools/seeded_random_rates.py [--log2 16 20] [--out profiles/r09_seeded_random.csv]
"""
import argparse
import csv
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RUNS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_seeded_random.csv"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bgn_amd
    import bgn_ref as R
    from bgn_amd._lib import check
    opk, _ = R.NewKeyGen(1024, 1021, 3, True, 1)                        # p of 1031 bits: L = 129
    p, n = opk.p, opk.n
    pk = bgn_amd.PublicKey(p, n, opk.l, R.elem_to_bytes(opk.P, p), R.elem_to_bytes(opk.Q, p), 1021)
    eng = pk.engine
    lib, E, nl = eng._lib, eng.elem_bytes, eng.n_len
    sync = torch.cuda.synchronize
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    seed = os.urandom(32)
    rows = []

    def record(what, count, ms, note=""):
        med, spread = statistics.median(ms), max(ms) - min(ms)
        rows.append([what, count, len(ms), "%.3f" % med, "%.3f" % spread, "%.4g" % (count / med * 1e3) if count else "", note])
        print(rows[-1], flush=True)
        return med, spread

    rng = random.Random(9)
    x_len = 8
    for lg in args.log2:
        N = 1 << lg
        x = np.frombuffer(rng.randbytes(N * x_len), dtype=np.uint8)
        out_b, out_c = np.zeros(N * E, dtype=np.uint8), np.zeros(N * E, dtype=np.uint8)

        def route_b():
            r = np.frombuffer(os.urandom(N * nl), dtype=np.uint8)
            check(lib.bgn_encrypt_batch(eng._h, N, ptr(x), x_len, ptr(r), nl, ptr(out_b)), "bgn_encrypt_batch")

        def route_c(t):
            check(lib.bgn_encrypt_seeded_batch(eng._h, N, ptr(x), x_len, seed, t, 0, ptr(out_c)), "bgn_encrypt_seeded_batch")

        route_b()                                                         # warm-up: window tables, workspace, staging
        route_c(0)
        tb, tc = [], []
        for run in range(RUNS):
            sync()
            t0 = time.perf_counter()
            route_b()
            t1 = time.perf_counter()
            route_c(run + 1)
            t2 = time.perf_counter()
            tb.append((t1 - t0) * 1e3)
            tc.append((t2 - t1) * 1e3)
        t0 = time.perf_counter()
        os.urandom(N * nl)
        draw_ms = (time.perf_counter() - t0) * 1e3
        mb, sb = record("encrypt_host_rows (b)", N, tb, "os.urandom of %d MB: %.1f ms of it" % (N * nl >> 20, draw_ms))
        mc, _ = record("encrypt_seeded (c)", N, tc)

        # (a) the expansion alone, device-resident
        rd = torch.zeros(N * nl, dtype=torch.uint8, device="cuda")
        eng.random_scalars_dev(rd, N, seed, 7, 0)
        sync()
        wall, ev = [], []
        for run in range(RUNS):
            sync()
            t0 = time.perf_counter()
            eng.random_scalars_dev(rd, N, seed, 8 + run, 0)
            sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(eng.last_kernel_ms())
        record("random_scalars_dev (a, wall)", N, wall)
        ma, _ = record("k_random_scalars (a, HIP events)", N, ev, eng.last_kernel_name())
        rows.append(["summary", N, "", "", "", "",
                     "(b) - (c) = %.3f ms against 3 x spread of (b) = %.3f ms; (a) is %.2f %% of (c)" % (mb - mc, 3 * sb, 100 * ma / mc)])
        print(rows[-1], flush=True)
        del rd

    # (d) resources per limb count
    for name in ("toy64", "k256", "k512", "k1024", "k1024b", "k2048"):
        with open(os.path.join(ROOT, "tests", "golden", name + ".json")) as f:
            fx = json.load(f)
        e = bgn_amd.Engine(int(fx["p"], 16), int(fx["n"], 16), fx["l"], bytes.fromhex(fx["P"]), bytes.fromhex(fx["Q"]))
        e.set_memory_budget(1 << 30)
        rd = torch.zeros(64 * e.n_len, dtype=torch.uint8, device="cuda")
        e.random_scalars_dev(rd, 64, seed, 0, 0)
        sync()
        res = (ctypes.c_int64 * 4)()
        check(lib.bgn_last_kernel_resources(e._h, res), "bgn_last_kernel_resources")
        need = (e.p.bit_length() + 9 + 28) // 29
        nl_ = min(v for v in (3, 10, 19, 36, 37, 72) if v >= need)
        rows.append(["k_random_scalars resources", "", "", "", "", "",
                     "NL %d (%s): %d vector registers, %d scratch bytes per lane, %d LDS bytes, %d threads" % ((nl_, name) + tuple(res))])
        print(rows[-1], flush=True)
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["what", "count", "runs", "median_ms", "max_minus_min_ms", "per_second", "note"])
        w.writerows(rows)


if __name__ == "__main__":
    main()
