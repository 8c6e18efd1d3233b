#!/usr/bin/env python3
"""Rates of the two paths of the linear map (bgn_lincomb_batch_dev) on device-resident arrays of the 1024-bit fixture key,
timed with HIP events, five launches per figure after a warm-up, in one process: the table path (lin_buckets = 0, which
is the call as it was before the bucket path), the bucket path (lin_buckets = 1, window and run planned), the planned
call, and bgn_sum_batch_dev of the same array — the floor no weighted sum can beat.  All three maps must agree byte for
byte.  Every row carries the sort / reduce split of its last launch (last_aux_kernel_ms, last_kernel_ms).

Shapes (nvec, nrows, d, w_bits): 1 x 1 x 2^20 at 8 and 16 bits, 1 x 4 x 2^18, 1 x 64 x 2^14 and 1 x 1024 x 1024 at 16 bits,
on both levels; --sweep also times the first 16-bit shape under lin_bucket_window 4 .. 8 and lin_bucket_run 4 .. 32.
A gain counts when it exceeds three times the larger max - min of the two series.
Writes a CSV (default profiles/r14_bucket_lincomb_rates.csv)."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1, 1 << 20, 8), (1, 1, 1 << 20, 16), (1, 4, 1 << 18, 16), (1, 64, 1 << 14, 16), (1, 1024, 1024, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key", default="k1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--shapes", default="0,1,2,3,4", help="indices into the shape list")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_bucket_lincomb_rates.csv"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import engine_key, load_fixture
    fx = load_fixture(args.key)
    eng = engine_key(fx)[0].engine
    E = eng.elem_bytes
    rng = np.random.default_rng(14)
    l1 = eng.encrypt([int(v) for v in rng.integers(1, 1 << 40, size=1024)])
    l2 = eng.mult(l1[:256].tobytes(), l1[256:512].tobytes())
    rows = []

    def timed(fn):
        ms = []
        for _ in range(args.reps + 1):                                     # the first launch warms the workspace up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms[1:]

    def report(what, level, shape, ms, note=""):
        med = sorted(ms)[len(ms) // 2]
        nvec, nrows, d, wb = shape
        row = {"what": what, "level": level, "nvec": nvec, "nrows": nrows, "d": d, "w_bits": wb, "ms_median": "%.4f" % med,
               "ms_min": "%.4f" % min(ms), "ms_max": "%.4f" % max(ms), "aux_ms": "%.4f" % eng.last_aux_kernel_ms(),
               "aux_kernel": eng.last_aux_kernel_name(), "kernel_ms": "%.4f" % eng.last_kernel_ms(),
               "kernel": eng.last_kernel_name(), "scratch": eng.last_kernel_resources()["scratch_bytes_per_lane"], "note": note}
        rows.append(row)
        print(row, flush=True)
        return med, max(ms) - min(ms)

    for level in [int(v) for v in args.levels.split(",")]:
        pool = l1 if level == 1 else l2
        for si in [int(v) for v in args.shapes.split(",")]:
            shape = SHAPES[si]
            nvec, nrows, d, wb = shape
            ct_h = pool[rng.integers(0, len(pool), size=nvec * d)]
            W = rng.integers(-(1 << wb) + 1, 1 << wb, size=(nrows, d), dtype=np.int64).astype(np.int32)
            ct = torch.from_numpy(ct_h.copy()).cuda().reshape(-1)
            w = torch.from_numpy(W).cuda()
            out = torch.zeros(nvec * nrows * E, dtype=torch.uint8, device="cuda")
            call = lambda: eng.lincomb_dev(level, ct, w, wb, out, nvec, nrows, d)
            eng.set_option("lin_buckets", 0)
            t_med, t_spread = report("tables", level, shape, timed(call), "lin_buckets 0")
            want = out.cpu().numpy().tobytes()
            eng.set_option("lin_buckets", 1)
            b_med, b_spread = report("buckets", level, shape, timed(call), "lin_buckets 1")
            assert out.cpu().numpy().tobytes() == want, "the two paths differ on level %d, shape %s" % (level, shape)
            eng.set_option("lin_buckets", -1)
            report("planned", level, shape, timed(call), "lin_buckets -1")
            assert out.cpu().numpy().tobytes() == want
            one = torch.zeros(nvec * E, dtype=torch.uint8, device="cuda")
            report("sum of the array", level, shape, timed(lambda: eng.sum_dev(level, ct, one, nvec, d)))
            noise = 3 * max(t_spread, b_spread)
            verdict = "gain" if t_med - b_med > noise else ("slower" if b_med - t_med > noise else "within noise")
            rows.append(dict.fromkeys(rows[0], ""))
            rows[-1].update({"what": "verdict: buckets %s, %.2f x" % (verdict, t_med / b_med), "level": level, "nvec": nvec,
                             "nrows": nrows, "d": d, "w_bits": wb, "ms_median": "%.4f" % (t_med - b_med), "ms_max": "%.4f" % noise,
                             "note": "bytes agree"})
            print(rows[-1], flush=True)
            if args.sweep and si == 1:
                eng.set_option("lin_buckets", 1)
                for opt, vals in (("lin_bucket_window", (4, 5, 6, 7, 8)), ("lin_bucket_run", (4, 8, 16, 32))):
                    for v in vals:
                        eng.set_option(opt, v)
                        report("buckets", level, shape, timed(call), "%s %d" % (opt, v))
                        assert out.cpu().numpy().tobytes() == want
                    eng.set_option(opt, -1)
            eng.reset_options()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        wr.writeheader()
        wr.writerows(rows)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
