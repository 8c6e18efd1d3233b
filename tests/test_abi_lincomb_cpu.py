"""CPU: the two linear-map entry points of include/bgn_amd.h (bgn_lincomb_batch and its `_dev` twin) are exported,
bound by the ctypes table, documented, and refuse bad arguments with BGN_E_ARG before any device is touched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAMES = ["bgn_lincomb_batch", "bgn_lincomb_batch_dev"]
BGN_E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from bgn_amd import _lib
    return _lib.load()


def test_the_two_symbols_are_exported_and_bound(lib):
    from bgn_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.PROTOTYPES and getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1], n
    host = _lib.PROTOTYPES["bgn_lincomb_batch"][1]
    assert _lib.PROTOTYPES["bgn_lincomb_batch_dev"][1] == host + [ctypes.c_void_p]
    # ctx, nvec, nrows, d, level, ct, w, w_bits, r, r_len, out
    assert host[1:5] == [ctypes.c_size_t] * 3 + [ctypes.c_int] and host[7] == ctypes.c_int and len(host) == 11


def test_the_header_says_what_the_call_promises():
    src = open(os.path.join(ROOT, "include", "bgn_amd.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int bgn_lincomb_batch\(", src, re.S)
    assert m, "bgn_lincomb_batch has no comment in front of it"
    doc = " ".join(re.sub(r"\n \*", "\n", m.group(1)).split())
    for promise in ("bgn.go:253-291", "bgn.go:442-497", "must not overlap", "mod 2^w_bits", "4-byte aligned", "2^28",
                    "bgn_neg_batch", "a row of zeros"):
        assert promise in doc, promise


def test_bad_arguments_are_refused_without_a_device(lib):
    """A null context is refused first, with a message, whatever the other arguments are, and nothing is written."""
    ct = ctypes.create_string_buffer(b"\x11" * 64, 64)
    w = (ctypes.c_int32 * 4)(1, -2, 3, 0)
    out = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    r = ctypes.create_string_buffer(8)
    good = (1, 2, 2, 1, ct, w, 8, None, 0, out)
    cases = [good]
    for at, bad in [(0, 0), (1, 0), (2, 0), (3, 0), (3, 3), (6, 0), (6, 32), (4, None), (5, None), (9, None), (7, r),
                    (0, 1 << 27), (1, 1 << 27), (2, 1 << 28), (0, (1 << 64) - 1)]:
        cases.append(good[:at] + (bad,) + good[at + 1:])
    for args in cases:
        assert lib.bgn_lincomb_batch(None, *args) == BGN_E_ARG, args[:4]
        assert lib.bgn_last_error()
        assert lib.bgn_lincomb_batch_dev(None, *args, None) == BGN_E_ARG, args[:4]
    assert out.raw == b"\x5a" * 64 and ct.raw == b"\x11" * 64 and list(w) == [1, -2, 3, 0]
