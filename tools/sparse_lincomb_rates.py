#!/usr/bin/env python3
"""Rates of the sparse linear map (bgn_sparse_lincomb_batch_dev) on device-resident arrays of the 1024-bit fixture key,
timed with HIP events: medians of five launches after a warm-up, in one process, the call and the route existing calls
offer for the same result alternating, the bytes of the two compared.

Shapes, on both levels:
  window   16 taps of 8-bit weights, 2^20 outputs from one vector of 2^20 + 15 elements — against sixteen
           bgn_multconst_batch_dev on offset views and fifteen bgn_add_batch_dev (the dense call cannot take the shape)
  sparse   1024 x 1024, 16 nonzeros per row, 16-bit weights — against bgn_lincomb_batch_dev on the densified matrix;
           with --sweep also under every lin_window
  groups   2^20 inputs into 4096 equal groups, unit weights — against bgn_sum_batch_dev on the grouped array
  permuted the same groups over a random permutation of the inputs, which no existing call serves (no alternative)
A difference counts as a gain only when it exceeds three times the larger max - min of the two series (DESIGN.md
section 10).  Writes a CSV (default profiles/r13_sparse_lincomb_rates.csv)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--shapes", default="window,sparse,groups,permuted")
    ap.add_argument("--log2", type=int, default=20, help="log2 of the outputs of `window` and of the inputs of `groups`")
    ap.add_argument("--sweep", action="store_true", help="also time `sparse` under every lin_window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_sparse_lincomb_rates.csv"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import engine_key, load_fixture
    eng = engine_key(load_fixture(args.key))[0].engine
    E = eng.elem_bytes
    rng = np.random.default_rng(13)
    l1 = eng.encrypt([int(v) for v in rng.integers(1, 1 << 40, size=1024)])
    l2 = eng.mult(l1[:256].tobytes(), l1[256:512].tobytes())
    N = 1 << args.log2
    rows = []
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64).astype(np.uint32).view(np.int32)).cuda()

    def timed(fns):
        """One series per function, the functions taking turns; the first round warms the workspaces up."""
        ms = [[] for _ in fns]
        for _ in range(args.reps + 1):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[i].append(a.elapsed_time(b))
        return [m[1:] for m in ms]

    def report(what, level, shape, nnz, ms, note=""):
        med = sorted(ms)[len(ms) // 2]
        row = {"what": what, "level": level, "shape": shape, "nnz": nnz, "ms_median": "%.4f" % med, "ms_min": "%.4f" % min(ms),
               "ms_max": "%.4f" % max(ms), "entries_per_s": "%.4g" % (nnz / (med * 1e-3)), "note": note}
        rows.append(row)
        print(row, flush=True)
        return med, max(ms) - min(ms)

    for level in [int(v) for v in args.levels.split(",")]:
        pool = l1 if level == 1 else l2
        for shape in args.shapes.split(","):
            alt, alt_name = None, ""
            if shape == "window":
                nrows, d, taps, wb = N, N + 15, 16, 8
                rp, col = taps * np.arange(nrows + 1), (np.arange(nrows)[:, None] + np.arange(taps)).reshape(-1)
                tw = rng.integers(1, 1 << wb, size=taps)
                w = np.tile(tw, nrows)
            elif shape == "sparse":
                nrows, d, taps, wb = 1024, 1024, 16, 16
                rp = taps * np.arange(nrows + 1)
                col = np.concatenate([np.sort(rng.choice(d, size=taps, replace=False)) for _ in range(nrows)])
                w = rng.integers(1, 1 << wb, size=nrows * taps)
            else:
                nrows, d, taps, wb = 4096, N, N // 4096, 1
                rp, w = taps * np.arange(nrows + 1), np.ones(N, dtype=np.int64)
                col = np.arange(N) if shape == "groups" else rng.permutation(N)
            nnz = len(col)
            ct_h = pool[rng.integers(0, len(pool), size=d)]
            ct = torch.from_numpy(ct_h.copy()).cuda().reshape(-1)
            d_rp, d_col, d_w = dev(rp), dev(col), dev(w)
            out = torch.zeros(nrows * E, dtype=torch.uint8, device="cuda")
            base = torch.zeros_like(out)
            new = lambda: eng.sparse_lincomb_dev(level, ct, d_rp, d_col, d_w, wb, out, 1, nrows, d, nnz, taps)
            if shape == "window":
                ks = [torch.full((nrows,), int(k), dtype=torch.uint8, device="cuda") for k in tw]
                tmp = torch.empty_like(out)

                def alt():
                    for t in range(taps):
                        view = ct[t * E:(t + nrows) * E]
                        eng.multconst_dev(level, view, ks[t], 1, base if t == 0 else tmp, nrows)
                        if t:
                            eng.add_dev(level, base, tmp, base, nrows)
                alt_name = "16 multconst + 15 add on offset views"
            elif shape == "sparse":
                W = np.zeros((nrows, d), dtype=np.int32)
                W[np.repeat(np.arange(nrows), taps), col] = w
                d_W = torch.from_numpy(W).cuda()
                alt = lambda: eng.lincomb_dev(level, ct, d_W, wb, base, 1, nrows, d)
                alt_name = "lincomb on the densified matrix"
            elif shape == "groups":
                alt = lambda: eng.sum_dev(level, ct, base, nrows, taps)
                alt_name = "sum on the grouped array"
            label = "%s %d x %d, %d per row, %d bits" % (shape, nrows, d, taps, wb)
            ms = timed([new, alt] if alt else [new])
            n_med, n_spread = report("sparse_lincomb", level, label, nnz, ms[0], "planned")
            if alt:
                a_med, a_spread = report(alt_name, level, label, nnz, ms[1])
                assert base.cpu().numpy().tobytes() == out.cpu().numpy().tobytes(), "the two routes differ: %s level %d" % (shape, level)
                noise = 3 * max(n_spread, a_spread)
                verdict = "gain" if a_med - n_med > noise else ("slower" if n_med - a_med > noise else "within noise")
                rows.append(dict.fromkeys(rows[0], ""))
                rows[-1].update({"what": "verdict: %s, %.2f x" % (verdict, a_med / n_med), "level": level, "shape": label,
                                 "ms_median": "%.4f" % (a_med - n_med), "ms_max": "%.4f" % noise, "note": "bytes agree"})
                print(rows[-1], flush=True)
            if args.sweep and shape == "sparse":
                got = out.cpu().numpy().tobytes()
                for omega in range(1, 9):
                    eng.set_option("lin_window", omega)
                    ms = timed([new])
                    assert out.cpu().numpy().tobytes() == got
                    report("sparse_lincomb", level, label, nnz, ms[0], "lin_window %d; aux %.4f ms, walk %.4f ms" %
                           (omega, eng.last_aux_kernel_ms(), eng.last_kernel_ms()))
                eng.reset_options()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        wr.writeheader()
        wr.writerows(rows)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
