"""CPU: the six proof entry points of include/bgn_amd.h (challenge, prove, verify, each with a `_dev` twin) are
exported, bound by the ctypes table, and refuse bad arguments with BGN_E_ARG before any device is touched."""
import ctypes

import pytest

NAMES = ["bgn_challenge_batch", "bgn_prove_plaintext_knowledge_batch", "bgn_verify_plaintext_knowledge_batch",
         "bgn_challenge_batch_dev", "bgn_prove_plaintext_knowledge_batch_dev", "bgn_verify_plaintext_knowledge_batch_dev"]
BGN_E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from bgn_amd import _lib
    return _lib.load()


def test_the_six_symbols_are_exported_and_bound(lib):
    from bgn_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.PROTOTYPES and getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1], n
    # a `_dev` twin takes its host form's arguments and a stream
    for n in NAMES[:3]:
        assert _lib.PROTOTYPES[n + "_dev"][1] == _lib.PROTOTYPES[n][1] + [ctypes.c_void_p], n


def test_bad_arguments_are_refused_without_a_device(lib):
    """No context exists on a machine without a GPU, and none is needed: a null context and null arrays are refused
    first, with a message, and nothing is written."""
    buf = ctypes.create_string_buffer(64)
    sentinel = bytes(buf.raw)
    calls = {
        "bgn_challenge_batch": (None, 1, buf, buf, buf),
        "bgn_challenge_batch_dev": (None, 1, buf, buf, buf, None),
        "bgn_prove_plaintext_knowledge_batch": (None, 1, buf, 8, buf, 8, buf, 8, buf, 8, buf, buf, buf),
        "bgn_prove_plaintext_knowledge_batch_dev": (None, 1, buf, 8, buf, 8, buf, 8, buf, 8, buf, buf, buf, None),
        "bgn_verify_plaintext_knowledge_batch": (None, 1, buf, buf, buf, buf, 8, buf),
        "bgn_verify_plaintext_knowledge_batch_dev": (None, 1, buf, buf, buf, buf, 8, buf, None),
    }
    assert sorted(calls) == sorted(NAMES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == BGN_E_ARG, name
        assert b"null" in lib.bgn_last_error(), name
        # count = 0 with a null context is still an argument error, not a silent success
        assert getattr(lib, name)(None, 0, *args[2:]) == BGN_E_ARG, name
    assert buf.raw == sentinel
