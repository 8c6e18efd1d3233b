"""The compressed wire form on device-resident arrays of a 1024-bit key (k1024), both levels, 2^16 and 2^20 elements:
k_compress_wire beside k_neg_wire (bytes moved / kernel time against the 8 TB/s HBM peak), k_decompress beside
MultConst level 1 with 1024-bit scalars, and upload + decompress against the upload of the full form.  Kernel ms by
the engine's HIP events over five launches after one warm-up: median and max - min.
   python tools/compress_rates.py [out.csv]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from conftest import load_fixture, engine_key

fx = load_fixture("k1024")
pk, _ = engine_key(fx)
eng = pk.engine
EB, CB = eng.elem_bytes, eng.L + 1
dev = torch.device("cuda", 0)
rows = []


def emit(*cols):
    rows.append(",".join(str(c) for c in cols))
    print(rows[-1], flush=True)


def timed(call, reps=5):
    call(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        call(); torch.cuda.synchronize()
        ms.append(eng.last_kernel_ms())
    return statistics.median(ms), max(ms) - min(ms)


def tiled(elems, n):
    pool = torch.frombuffer(bytearray(b"".join(elems)), dtype=torch.uint8).view(len(elems), -1).to(dev)
    return pool[torch.arange(n, device=dev) % len(elems)].contiguous().view(-1)


emit("what", "level", "log2", "kernel_ms_median", "kernel_ms_spread", "per_s", "bytes_per_elem", "frac_of_8TBps")
l1 = [bytes.fromhex(e["ct"]) for e in fx["encrypt"]]
l2 = [bytes.fromhex(v["out"]) for v in fx["mult"]]
for lg in (16, 20):
    n = 1 << lg
    for level, elems in ((1, l1), (2, l2)):
        a = tiled(elems, n)
        c = torch.empty(n * CB, dtype=torch.uint8, device=dev)
        o = torch.empty(n * EB, dtype=torch.uint8, device=dev)
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        for name, nbytes, call in (("k_neg_wire", 2 * EB, lambda: eng.neg_dev(level, a, o, n)),
                                   ("k_compress_wire", EB + CB, lambda: eng.compress_dev(level, a, c, n)),
                                   ("k_decompress", CB + EB + 1, lambda: eng.decompress_dev(level, c, o, ok, n))):
            med, spread = timed(call)
            assert eng.last_kernel_name() == name
            emit(name, level, lg, "%.4f" % med, "%.4f" % spread, "%.4e" % (n / (med * 1e-3)), nbytes,
                 "%.3f" % (nbytes * n / (med * 1e-3) / 8e12))
        assert bool((o == a).all().item()) and bool((ok == 1).all().item())
        del a, c, o, ok
# the comparison: MultConst level 1, 1024-bit scalars, 2^16 (the only other thousand-step chain per element)
n = 1 << 16
a = tiled(l1, n)
o = torch.empty(n * EB, dtype=torch.uint8, device=dev)
g = torch.Generator(device="cpu"); g.manual_seed(16)
k = torch.randint(0, 256, (n * 128,), dtype=torch.uint8, generator=g).to(dev)
med, spread = timed(lambda: eng.multconst_dev(1, a, k, 128, o, n), reps=3)
emit(eng.last_kernel_name() + " (MultConst 1024-bit)", 1, 16, "%.4f" % med, "%.4f" % spread, "%.4e" % (n / (med * 1e-3)), "", "")
# end to end from pinned host memory, 2^20 level 1: upload + decompress against the upload of the full form
n = 1 << 20
full = tiled(l1, n)
comp = torch.empty(n * CB, dtype=torch.uint8, device=dev)
eng.compress_dev(1, full, comp, n)
h_full, h_comp = full.cpu().pin_memory(), comp.cpu().pin_memory()
ok = torch.empty(n, dtype=torch.uint8, device=dev)
for name, run in (("upload full form", lambda: full.copy_(h_full, non_blocking=True)),
                  ("upload compressed + k_decompress", lambda: (comp.copy_(h_comp, non_blocking=True), eng.decompress_dev(1, comp, full, ok, n)))):
    ts = []
    for _ in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        run(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[1:]
    emit(name + " (wall ms)", 1, 20, "%.3f" % statistics.median(ts), "%.3f" % (max(ts) - min(ts)), "%.4e" % (n / (statistics.median(ts) * 1e-3)), "", "")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(rows) + "\n")
