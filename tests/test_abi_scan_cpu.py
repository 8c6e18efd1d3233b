"""CPU: bgn_scan_batch and its `_dev` twin refuse a null context with BGN_E_ARG before any device is touched, whatever
the other arguments (the refusals behind that check need a context: the GPU suite's C twin makes them); and the
planning of the recursion (dispatch.hpp plan_scan) holds its properties — tests/cpp/scan_plan_test.cpp, a stand-alone
program built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import subprocess

from conftest import ROOT


def test_a_null_context_is_refused_first_and_nothing_is_written():
    from bgn_amd import _lib
    lib = _lib.load()
    ct = ctypes.create_string_buffer(b"\x11" * 64, 64)
    out = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    r = ctypes.create_string_buffer(8)
    for args in [(1, 4, 1, ct, None, 0, out), (0, 4, 1, ct, None, 0, out), (1, 0, 1, ct, None, 0, out),
                 (1, 4, 3, ct, None, 0, out), (1, 4, 1, None, None, 0, None), (1, 4, 2, ct, r, 0, out),
                 (1 << 20, 1 << 20, 1, ct, None, 0, out)]:
        assert lib.bgn_scan_batch(None, *args) == -1, args[:3]
        assert lib.bgn_last_error()
        assert lib.bgn_scan_batch_dev(None, *args, None) == -1, args[:3]
    assert out.raw == b"\x5a" * 64 and ct.raw == b"\x11" * 64


def test_the_planner_holds_its_properties():
    src = os.path.join(ROOT, "tests", "cpp", "scan_plan_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "scan_plan_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
