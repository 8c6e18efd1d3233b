"""CPU: the two segmented-sum entry points of include/bgn_amd.h (bgn_sum_batch and its `_dev` twin) are exported,
bound by the ctypes table, and refuse bad arguments with BGN_E_ARG before any device is touched."""
import ctypes

import pytest

NAMES = ["bgn_sum_batch", "bgn_sum_batch_dev"]
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
    host = _lib.PROTOTYPES["bgn_sum_batch"][1]
    assert _lib.PROTOTYPES["bgn_sum_batch_dev"][1] == host + [ctypes.c_void_p]
    # ctx, nseg, seg_len, level, ct, r, r_len, out
    assert host[1:4] == [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int] and len(host) == 8


def test_the_header_says_what_the_call_promises():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bgn_amd.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int bgn_sum_batch\(", src, re.S)
    assert m, "bgn_sum_batch has no comment in front of it"
    doc = " ".join(m.group(1).split())
    assert "bgn.go:442-497" in doc and "must not overlap" in doc


def test_bad_arguments_are_refused_without_a_device(lib):
    """No context exists on a machine without a GPU, and none is needed: a null context is refused first, with a
    message, whatever the other arguments are, and nothing is written."""
    ct = ctypes.create_string_buffer(b"\x11" * 64, 64)
    out = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    r = ctypes.create_string_buffer(8)
    cases = [
        (1, 4, 1, ct, None, 0, out),          # a well-formed call: only the context is missing
        (0, 4, 1, ct, None, 0, out),          # nseg == 0
        (1, 0, 1, ct, None, 0, out),          # seg_len == 0
        (1, 4, 0, ct, None, 0, out),          # level
        (1, 4, 3, ct, None, 0, out),
        (1, 4, 1, None, None, 0, out),        # null pointers
        (1, 4, 1, ct, None, 0, None),
        (1, 4, 2, ct, r, 0, out),             # r without a length
        (1 << 20, 1 << 20, 1, ct, None, 0, out),   # nseg * seg_len above 2^28
        ((1 << 64) - 1, (1 << 64) - 1, 2, ct, None, 0, out),
    ]
    for args in cases:
        assert lib.bgn_sum_batch(None, *args) == BGN_E_ARG, args[:3]
        assert lib.bgn_last_error()
        assert lib.bgn_sum_batch_dev(None, *args, None) == BGN_E_ARG, args[:3]
    assert out.raw == b"\x5a" * 64 and ct.raw == b"\x11" * 64
