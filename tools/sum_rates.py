#!/usr/bin/env python3
"""Rates of the segmented sum (bgn_sum_batch_dev) on device-resident arrays of the 1024-bit fixture key, timed with
HIP events, five launches per figure, in one process:

  * 1 x 2^20 on both levels against the only alternative without the call: the halving tree of bgn_add_batch_dev on
    the same array (twenty launches, a = first half, b = second half, in place);
  * 4096 x 256 and 65536 x 16, which no tree of contiguous Adds can serve, as elements per second.

Prints every figure and writes them to a CSV (default profiles/r10_sum_rates.csv).  The sum and the tree must agree
byte for byte; a gain counts when it exceeds three times the larger max - min of the two series.
"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key", default="k1024")
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="also time 1 x N under other settings of sum_lanes / sum_run_min")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_sum_rates.csv"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import engine_key, load_fixture
    fx = load_fixture(args.key)
    pk, _ = engine_key(fx)
    eng = pk.engine
    E = eng.elem_bytes
    N = 1 << args.log2
    rng = np.random.default_rng(10)
    xs = [int(v) for v in rng.integers(1, 1 << 40, size=1024)]
    l1 = eng.encrypt(xs)                                                   # 1024 level-1 ciphertexts
    l2 = eng.mult(l1[:256].tobytes(), l1[256:512].tobytes())               # 256 level-2 ciphertexts
    rows = []

    def timed(fn, prep=None):
        ms = []
        for _ in range(args.reps + 1):                                     # the first launch warms the workspace up
            if prep:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms[1:]

    def report(what, level, nseg, seg_len, ms):
        med = sorted(ms)[len(ms) // 2]
        row = {"what": what, "level": level, "nseg": nseg, "seg_len": seg_len, "ms_median": "%.4f" % med,
               "ms_min": "%.4f" % min(ms), "ms_max": "%.4f" % max(ms), "elements_per_s": "%.4g" % (nseg * seg_len / (med * 1e-3)),
               "kernel": eng.last_kernel_name()}
        rows.append(row)
        print(row, flush=True)
        return med, max(ms) - min(ms)

    for level, pool in ((1, l1), (2, l2)):
        reps = -(-N // len(pool))
        master = torch.from_numpy(np.tile(pool, (reps, 1))[:N].copy()).cuda().reshape(-1)
        work = torch.empty_like(master)
        out = torch.zeros(65536 * E, dtype=torch.uint8, device="cuda")
        # the sum, 1 x N
        ms_sum = timed(lambda: eng.sum_dev(level, master, out, 1, N))
        got_sum = out[:E].cpu().numpy().tobytes()
        s_med, s_spread = report("sum", level, 1, N, ms_sum)

        def tree():
            h = N // 2
            while h >= 1:
                eng.add_dev(level, work[:h * E], work[h * E:2 * h * E], work[:h * E], h)
                h //= 2
        ms_tree = timed(tree, prep=lambda: work.copy_(master))
        got_tree = work[:E].cpu().numpy().tobytes()
        t_med, t_spread = report("tree of add_dev", level, 1, N, ms_tree)
        assert got_sum == got_tree, "the sum and the tree of Adds differ on level %d" % level
        noise = 3 * max(s_spread, t_spread)
        verdict = "gain" if t_med - s_med > noise else ("slower" if s_med - t_med > noise else "within noise")
        print("level %d, 1 x 2^%d: sum %.3f ms, tree %.3f ms, 3 x spread %.3f ms: %s" % (level, args.log2, s_med, t_med, noise, verdict), flush=True)
        rows.append({"what": "verdict: " + verdict, "level": level, "nseg": 1, "seg_len": N, "ms_median": "%.4f" % (t_med - s_med),
                     "ms_min": "", "ms_max": "%.4f" % noise, "elements_per_s": "", "kernel": ""})
        if args.sweep:                                                     # the planner's two knobs at 1 x N
            for lanes in (65536, 131072, 262144, 524288):
                for run_min in (2, 4, 8, 16):
                    eng.set_option("sum_lanes", lanes)
                    eng.set_option("sum_run_min", run_min)
                    ms = timed(lambda: eng.sum_dev(level, master, out, 1, N))
                    assert out[:E].cpu().numpy().tobytes() == got_sum
                    report("sum lanes=%d run_min=%d" % (lanes, run_min), level, 1, N, ms)
            eng.reset_options()
        # shapes the tree cannot serve
        for nseg, seg_len in ((4096, 256), (65536, 16)):
            if nseg * seg_len > N:
                continue
            ms = timed(lambda: eng.sum_dev(level, master, out, nseg, seg_len))
            report("sum", level, nseg, seg_len, ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows(rows)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
