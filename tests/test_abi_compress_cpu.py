"""CPU: the four entry points of the compressed wire form (bgn_compress_batch, bgn_decompress_batch and their `_dev`
twins) are exported, bound by the ctypes table, documented in include/bgn_amd.h, and refuse bad arguments with
BGN_E_ARG before any device is touched."""
import ctypes

import pytest

NAMES = ["bgn_compress_batch", "bgn_decompress_batch", "bgn_compress_batch_dev", "bgn_decompress_batch_dev"]
BGN_E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from bgn_amd import _lib
    return _lib.load()


def test_the_four_symbols_are_exported_and_bound(lib):
    from bgn_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.PROTOTYPES and getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1], n
    for host in NAMES[:2]:
        assert _lib.PROTOTYPES[host + "_dev"][1] == _lib.PROTOTYPES[host][1] + [ctypes.c_void_p]
    # ctx, count, level, in, out (, ok)
    assert [len(_lib.PROTOTYPES[n][1]) for n in NAMES[:2]] == [5, 6]
    assert _lib.PROTOTYPES[NAMES[0]][1][1:3] == [ctypes.c_size_t, ctypes.c_int]


def test_the_header_states_the_format():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "bgn_amd.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int bgn_compress_batch\(", src, re.S)
    assert m, "bgn_compress_batch has no comment in front of it"
    doc = " ".join(m.group(1).split())
    for promise in ("fp_bytes + 1", "0x02", "must not overlap", "not pinned", "2^28"):
        assert promise in doc, promise


def test_bad_arguments_are_refused_without_a_device(lib):
    """No context exists on a machine without a GPU, and none is needed: a null context is refused first, whatever the
    other arguments are, and nothing is written."""
    src = ctypes.create_string_buffer(b"\x11" * 64, 64)
    out = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    ok = ctypes.create_string_buffer(b"\x5a" * 8, 8)
    cases = [
        (1, 1, src, out),                 # a well-formed call: only the context is missing
        (0, 1, src, out),                 # count == 0
        (1, 0, src, out),                 # level
        (1, 3, src, out),
        (1, 1, None, out),                # null pointers
        (1, 2, src, None),
        ((1 << 28) + 1, 1, src, out),     # count above 2^28
        ((1 << 64) - 1, 2, src, out),
    ]
    for args in cases:
        assert lib.bgn_compress_batch(None, *args) == BGN_E_ARG, args[:2]
        assert lib.bgn_last_error()
        assert lib.bgn_compress_batch_dev(None, *args, None) == BGN_E_ARG, args[:2]
        assert lib.bgn_decompress_batch(None, *args, ok) == BGN_E_ARG, args[:2]
        assert lib.bgn_decompress_batch_dev(None, *args, ok, None) == BGN_E_ARG, args[:2]
    assert lib.bgn_decompress_batch(None, 1, 1, src, out, None) == BGN_E_ARG
    assert out.raw == b"\x5a" * 64 and src.raw == b"\x11" * 64 and ok.raw == b"\x5a" * 8
