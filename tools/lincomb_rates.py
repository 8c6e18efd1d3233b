#!/usr/bin/env python3
"""Rates of the linear map (bgn_lincomb_batch_dev) on device-resident arrays of the 1024-bit fixture key, timed with HIP
events, five launches per figure after a warm-up, in one process, against the route available without the call: the
vector replicated once per row, bgn_multconst_batch_dev with k_len bytes per weight, bgn_sum_batch_dev with
seg_len = d.  Both routes must agree byte for byte (the weights are non-negative: MultConst takes no sign).

Shapes (nvec, nrows, d, w_bits): 1 x 1024 x 1024 at 16 and 8 bits, 64 x 16 x 256 at 8 bits, 1 x 1 x 2^20 at 16 bits, on
both levels; with --sweep also every lin_window at the first shape.  Every row carries the table / walk split of its
last launch (last_aux_kernel_ms: digit planes + tables; last_kernel_ms: walk + encoding + the fold of the chunks).
A gain counts when it exceeds three times the larger max - min of the two series.
Writes a CSV (default profiles/r11_lincomb_rates.csv)."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1024, 1024, 16), (1, 1024, 1024, 8), (64, 16, 256, 8), (1, 1, 1 << 20, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key", default="k1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--sweep", action="store_true", help="also time the first shape under every lin_window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_lincomb_rates.csv"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import engine_key, load_fixture
    fx = load_fixture(args.key)
    eng = engine_key(fx)[0].engine
    E = eng.elem_bytes
    rng = np.random.default_rng(11)
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
               "ms_min": "%.4f" % min(ms), "ms_max": "%.4f" % max(ms), "entries_per_s": "%.4g" % (nvec * nrows * d / (med * 1e-3)),
               "aux_ms": "%.4f" % eng.last_aux_kernel_ms(), "aux_kernel": eng.last_aux_kernel_name(),
               "kernel_ms": "%.4f" % eng.last_kernel_ms(), "kernel": eng.last_kernel_name(), "note": note}
        rows.append(row)
        print(row, flush=True)
        return med, max(ms) - min(ms)

    for level in [int(v) for v in args.levels.split(",")]:
        pool = l1 if level == 1 else l2
        for si in [int(v) for v in args.shapes.split(",")]:
            shape = SHAPES[si]
            nvec, nrows, d, wb = shape
            ct_h = pool[rng.integers(0, len(pool), size=nvec * d)]
            W = rng.integers(0, 1 << wb, size=(nrows, d), dtype=np.int64).astype(np.int32)
            ct = torch.from_numpy(ct_h.copy()).cuda().reshape(-1)
            w = torch.from_numpy(W).cuda()
            out = torch.zeros(nvec * nrows * E, dtype=torch.uint8, device="cuda")
            ms_lin = timed(lambda: eng.lincomb_dev(level, ct, w, wb, out, nvec, nrows, d))
            got = out.cpu().numpy().tobytes()
            l_med, l_spread = report("lincomb", level, shape, ms_lin, "lin_window planned")
            # the route without the call: replicate, MultConst, Sum
            klen = (wb + 7) // 8
            rep = torch.from_numpy(np.tile(ct_h.reshape(nvec, 1, d * E), (1, nrows, 1)).copy()).cuda().reshape(-1)
            kb = np.zeros((nvec, nrows * d, klen), dtype=np.uint8)
            for b in range(klen):
                kb[:, :, klen - 1 - b] = ((W.reshape(-1).astype(np.int64) >> (8 * b)) & 0xFF).astype(np.uint8)
            k = torch.from_numpy(kb).cuda().reshape(-1)
            prod = torch.empty_like(rep)
            base = torch.zeros_like(out)

            def route():
                eng.multconst_dev(level, rep, k, klen, prod, nvec * nrows * d)
                eng.sum_dev(level, prod, base, nvec * nrows, d)
            ms_base = timed(route)
            b_med, b_spread = report("multconst + sum", level, shape, ms_base, "k_len %d" % klen)
            assert base.cpu().numpy().tobytes() == got, "the two routes differ on level %d, shape %s" % (level, shape)
            noise = 3 * max(l_spread, b_spread)
            verdict = "gain" if b_med - l_med > noise else ("slower" if l_med - b_med > noise else "within noise")
            rows.append(dict.fromkeys(rows[0], ""), )
            rows[-1].update({"what": "verdict: %s, %.2f x" % (verdict, b_med / l_med), "level": level, "nvec": nvec, "nrows": nrows,
                             "d": d, "w_bits": wb, "ms_median": "%.4f" % (b_med - l_med), "ms_max": "%.4f" % noise,
                             "note": "bytes agree"})
            print(rows[-1], flush=True)
            del rep, prod, k
            if args.sweep and si == 0:
                for omega in range(1, 9):
                    eng.set_option("lin_window", omega)
                    ms = timed(lambda: eng.lincomb_dev(level, ct, w, wb, out, nvec, nrows, d))
                    assert out.cpu().numpy().tobytes() == got
                    report("lincomb", level, shape, ms, "lin_window %d" % omega)
                eng.reset_options()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        wr.writeheader()
        wr.writerows(rows)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
