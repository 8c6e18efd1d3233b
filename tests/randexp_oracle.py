"""Expansion 1 of include/bgn_amd.h in hashlib and Python integers (TEST INFRASTRUCTURE): what the seeded-randomness
tests compare the emulation, the kernels and the C caller against.  Nothing here calls the engine."""
import hashlib

SURPLUS = 16


def block(K: bytes, t: int, i: int, j: int) -> bytes:
    """B_j = SHA-256(K || be64(t) || be64(i) || be32(j))."""
    assert len(K) == 32
    return hashlib.sha256(K + t.to_bytes(8, "big") + i.to_bytes(8, "big") + j.to_bytes(4, "big")).digest()


def draw(K: bytes, t: int, i: int, n_len: int) -> int:
    """W: the first n_len + 16 bytes of B_0 || B_1 || ... as a big-endian integer."""
    wlen, s, j = n_len + SURPLUS, b"", 0
    while len(s) < wlen:
        s += block(K, t, i, j)
        j += 1
    return int.from_bytes(s[:wlen], "big")


def n_len_of(n: int) -> int:
    return (n.bit_length() + 7) // 8


def scalar(K: bytes, t: int, i: int, n: int) -> int:
    return draw(K, t, i, n_len_of(n)) % n


def scalars(K: bytes, t: int, first: int, count: int, n: int):
    return [scalar(K, t, first + e, n) for e in range(count)]


def rows(K: bytes, t: int, first: int, count: int, n: int) -> bytes:
    """The count rows of n_len bytes a call returns."""
    nl = n_len_of(n)
    return b"".join(r.to_bytes(nl, "big") for r in scalars(K, t, first, count, n))
