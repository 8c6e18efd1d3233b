"""CPU: the five seeded-randomness entry points of include/bgn_amd.h (random scalars and Encrypt from a seed, each with a
`_dev` twin, and the multi-device Encrypt) are exported, bound by the ctypes table, and refuse bad arguments with
BGN_E_ARG before any device is touched."""
import ctypes

import pytest

HOST = ["bgn_random_scalars_batch", "bgn_encrypt_seeded_batch"]
NAMES = HOST + [n + "_dev" for n in HOST] + ["bgn_mencrypt_seeded_batch"]
BGN_OK, BGN_E_ARG = 0, -1


@pytest.fixture(scope="module")
def lib():
    from bgn_amd import _lib
    return _lib.load()


def test_the_five_symbols_are_exported_and_bound(lib):
    from bgn_amd import _lib
    assert len(NAMES) == 5
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.PROTOTYPES and getattr(lib, n).argtypes == _lib.PROTOTYPES[n][1], n
    # a `_dev` twin takes its host form's arguments and a stream
    for n in HOST:
        assert _lib.PROTOTYPES[n + "_dev"][1] == _lib.PROTOTYPES[n][1] + [ctypes.c_void_p], n
    # the multi-device Encrypt takes what the single-device one takes
    assert _lib.PROTOTYPES["bgn_mencrypt_seeded_batch"][1][1:] == _lib.PROTOTYPES["bgn_encrypt_seeded_batch"][1][1:]
    # stream id and first index are 64-bit, in front of the output
    for n in HOST:
        assert _lib.PROTOTYPES[n][1][-3:-1] == [ctypes.c_uint64, ctypes.c_uint64], n


def test_bad_arguments_are_refused_without_a_device(lib):
    """No context exists on a machine without a GPU, and none is needed: a null context is refused first, with a
    message, whatever the other arguments are — a null seed, a null output, a zero x_len, count = 0 — and nothing is
    written."""
    buf = ctypes.create_string_buffer(64)
    seed = ctypes.create_string_buffer(32)
    sentinel = bytes(buf.raw)
    top = (1 << 64) - 1
    calls = {
        "bgn_random_scalars_batch": lambda **k: (None, k.get("count", 1), k.get("seed", seed), 0, k.get("first", 0), k.get("out", buf)),
        "bgn_random_scalars_batch_dev": lambda **k: (None, k.get("count", 1), k.get("seed", seed), 0, k.get("first", 0),
                                                     k.get("out", buf), None),
        "bgn_encrypt_seeded_batch": lambda **k: (None, k.get("count", 1), buf, k.get("x_len", 8), k.get("seed", seed), 0,
                                                 k.get("first", 0), k.get("out", buf)),
        "bgn_encrypt_seeded_batch_dev": lambda **k: (None, k.get("count", 1), buf, k.get("x_len", 8), k.get("seed", seed), 0,
                                                     k.get("first", 0), k.get("out", buf), None),
        "bgn_mencrypt_seeded_batch": lambda **k: (None, k.get("count", 1), buf, k.get("x_len", 8), k.get("seed", seed), 0,
                                                  k.get("first", 0), k.get("out", buf)),
    }
    assert sorted(calls) == sorted(NAMES)
    for name, args in calls.items():
        for bad in (dict(), dict(seed=None), dict(out=None), dict(x_len=0), dict(first=top, count=2), dict(count=0)):
            assert getattr(lib, name)(*args(**bad)) == BGN_E_ARG, (name, bad)
            assert lib.bgn_last_error(), (name, bad)
        assert getattr(lib, name)(*args()) == BGN_E_ARG and b"null" in lib.bgn_last_error(), name
    assert buf.raw == sentinel and seed.raw == bytes(32)
