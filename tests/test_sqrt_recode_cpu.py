"""CPU: the square root's exponent (p + 1) / 4 of every fixture key, recoded by csrc/sqrtrecode.hpp into the program
k_decompress walks, replays to the exponent — tests/cpp/sqrt_recode_test.cpp, a stand-alone program built with the
address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT, load_fixture

KEYS = ("toy64", "k256", "k512", "k1024", "k1024b", "k2048")


def test_the_program_replays_to_the_exponent_for_every_fixture_p():
    src = os.path.join(ROOT, "tests", "cpp", "sqrt_recode_test.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "sqrt_recode_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    ps = [load_fixture(k)["p"] for k in KEYS]
    r = subprocess.run([exe] + [p[2:] if p.startswith("0x") else p for p in ps], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == len(KEYS) + 1
