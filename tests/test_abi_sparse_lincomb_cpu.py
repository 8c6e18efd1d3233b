"""CPU: bgn_sparse_lincomb_batch and its `_dev` twin are exported and bound with the header's signature, and refuse a
null context with BGN_E_ARG before any device is touched, whatever the other arguments; and the planner (dispatch.hpp
plan_sparse_lincomb) holds its properties — tests/cpp/sparse_plan_test.cpp, a stand-alone program built with the address
and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

from conftest import ROOT


def test_the_two_symbols_are_exported_and_bound():
    from bgn_amd import _lib
    lib = _lib.load()
    host = _lib.PROTOTYPES["bgn_sparse_lincomb_batch"][1]
    assert _lib.PROTOTYPES["bgn_sparse_lincomb_batch_dev"][1] == host + [ctypes.c_void_p]
    for n in ("bgn_sparse_lincomb_batch", "bgn_sparse_lincomb_batch_dev"):
        assert getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1], n
    # ctx, nvec, nrows, d, nnz, row_max, level, ct, row_ptr, col, w, w_bits, r, r_len, out
    assert host[1:7] == [ctypes.c_size_t] * 5 + [ctypes.c_int] and host[11] == ctypes.c_int and len(host) == 15
    src = " ".join(open(os.path.join(ROOT, "include", "bgn_amd.h")).read().split())
    assert ("int bgn_sparse_lincomb_batch(bgn_ctx* ctx, size_t nvec, size_t nrows, size_t d, size_t nnz, size_t row_max, int level, "
            "const uint8_t* ct, const uint32_t* row_ptr, const uint32_t* col, const int32_t* w, int w_bits, "
            "const uint8_t* r_be, size_t r_len, uint8_t* out);") in src


def test_a_null_context_is_refused_first_and_nothing_is_written():
    from bgn_amd import _lib
    lib = _lib.load()
    ct = ctypes.create_string_buffer(b"\x11" * 64, 64)
    out = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    rp, col, w = (ctypes.c_uint32 * 3)(0, 1, 2), (ctypes.c_uint32 * 2)(0, 1), (ctypes.c_int32 * 2)(3, -4)
    good = (1, 2, 2, 2, 1, 1, ct, rp, col, w, 8, None, 0, out)
    for at, bad in [(0, 1), (0, 0), (1, 0), (2, 0), (4, 0), (5, 3), (10, 32), (6, None), (8, None), (13, None),
                    (11, ctypes.create_string_buffer(8)), (3, 1 << 40)]:
        args = good[:at] + (bad,) + good[at + 1:]
        assert lib.bgn_sparse_lincomb_batch(None, *args) == -1, (at, bad)
        assert lib.bgn_last_error()
        assert lib.bgn_sparse_lincomb_batch_dev(None, *args, None) == -1, (at, bad)
    assert out.raw == b"\x5a" * 64 and ct.raw == b"\x11" * 64 and list(w) == [3, -4]


def test_the_planner_holds_its_properties():
    src = os.path.join(ROOT, "tests", "cpp", "sparse_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "sparse_plan_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
