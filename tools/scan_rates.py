#!/usr/bin/env python3
"""Rates of the prefix sums (bgn_scan_batch_dev) on device-resident arrays of the 1024-bit fixture key, timed with HIP
events, medians of five launches after a warm-up, in one process: 1 x 2^20, 4096 x 256 and 65536 x 16 on both levels,
each against the only route without the call — the doubling scheme, ceil(log2 seg_len) full-size launches of
bgn_add_batch_dev over offset views of the same data (out[i] = in[i] + in[i - d], d = 1, 2, 4, ...; the first d
elements of every segment copied through), between two buffers.  The copies (one strided device copy per step) are
part of that route and of its time; their share is largest at 65536 x 16.

Prints every figure and writes them to a CSV (default profiles/r12_scan_rates.csv).  The two routes must agree byte
for byte; a gain counts when it exceeds three times the larger max - min of the two series.
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
    ap.add_argument("--sweep", action="store_true", help="also time 1 x N under forced scan_chunk values")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_scan_rates.csv"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import engine_key, load_fixture
    fx = load_fixture(args.key)
    pk, _ = engine_key(fx)
    eng = pk.engine
    E = eng.elem_bytes
    N = 1 << args.log2
    rng = np.random.default_rng(12)
    xs = [int(v) for v in rng.integers(1, 1 << 40, size=1024)]
    l1 = eng.encrypt(xs)                                                   # 1024 level-1 ciphertexts
    l2 = eng.mult(l1[:256].tobytes(), l1[256:512].tobytes())               # 256 level-2 ciphertexts
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
        out = torch.zeros_like(master)
        buf = [torch.empty_like(master), torch.empty_like(master)]
        for nseg, seg_len in ((1, N), (4096, 256), (65536, 16)):
            if nseg * seg_len != N:
                continue
            ms_scan = timed(lambda: eng.scan_dev(level, master, out, nseg, seg_len))
            s_med, s_spread = report("scan", level, nseg, seg_len, ms_scan)
            last = [master]

            def doubling():
                src, k, d = master, 0, 1
                while d < seg_len:
                    dst = buf[k]
                    eng.add_dev(level, src[d * E:], src[:(N - d) * E], dst[d * E:], N - d)
                    dst.view(nseg, seg_len, E)[:, :d].copy_(src.view(nseg, seg_len, E)[:, :d])
                    src, k, d = dst, k ^ 1, 2 * d
                last[0] = src
            ms_dbl = timed(doubling)
            d_med, d_spread = report("doubling scheme of add_dev", level, nseg, seg_len, ms_dbl)
            assert torch.equal(out, last[0]), "the scan and the doubling scheme differ on level %d, %d x %d" % (level, nseg, seg_len)
            noise = 3 * max(s_spread, d_spread)
            verdict = "gain" if d_med - s_med > noise else ("slower" if s_med - d_med > noise else "within noise")
            print("level %d, %d x %d: scan %.3f ms, doubling %.3f ms, 3 x spread %.3f ms: %s" %
                  (level, nseg, seg_len, s_med, d_med, noise, verdict), flush=True)
            rows.append({"what": "verdict: " + verdict, "level": level, "nseg": nseg, "seg_len": seg_len, "ms_median": "%.4f" % (d_med - s_med),
                         "ms_min": "", "ms_max": "%.4f" % noise, "elements_per_s": "", "kernel": ""})
        if args.sweep:
            for c in (4, 8, 16, 32, 64):
                eng.set_option("scan_chunk", c)
                ms = timed(lambda: eng.scan_dev(level, master, out, 1, N))
                report("scan scan_chunk=%d" % c, level, 1, N, ms)
            eng.reset_options()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        w.writeheader()
        w.writerows(rows)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
