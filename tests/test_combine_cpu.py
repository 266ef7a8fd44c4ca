"""kvsep_crc32c_combine (include/kvsep_crc32c.h): the CRC of A||B from the CRCs of its parts.  Host only, no GPU.

Against the oracle over real bytes -- combine(Extend(c, A), Value(B), |B|) == Extend(c, A||B) for every pair of lengths
around the word, row, page and 64 KiB edges -- and against polynomial arithmetic written out here in plain Python
integers, for lengths whose 8n no longer fits 64 bits."""
import numpy as np
import pytest

import kvsep
from kvsep import splitmix64_bytes

LENGTHS = [0, 1, 3, 4, 15, 16, 17, 255, 256, 257, 1023, 1024, 4095, 4096, 4097, 65535, (1 << 20) + 1]
MID = max(LENGTHS)


@pytest.fixture(scope="module")
def parts(oracle):
    """A = the la bytes before MID, B = the lb bytes after it, so A||B is one contiguous range for the oracle."""
    data = splitmix64_bytes(2 * MID, 20261020, 0)
    value_b = {lb: oracle.extend_addr(0, data.ctypes.data + MID, lb) for lb in LENGTHS}
    return data, value_b


@pytest.mark.parametrize("crc_a_seed", [None, 0x9E3779B9, 0xFFFFFFFF])
def test_combine_matches_extend_over_the_concatenation(oracle, parts, crc_a_seed):
    data, value_b = parts
    base = data.ctypes.data
    for k, la in enumerate(LENGTHS):
        c = 0 if crc_a_seed is None else (crc_a_seed * (2 * k + 1)) & 0xFFFFFFFF
        ext_a = oracle.extend_addr(c, base + MID - la, la)
        for lb in LENGTHS:
            want = oracle.extend_addr(c, base + MID - la, la + lb)
            assert kvsep.combine(ext_a, value_b[lb], lb) == want, (c, la, lb)


def test_empty_b_returns_crc_a():
    for c in (0, 1, 0x80000000, 0xDEADBEEF, 0xFFFFFFFF):
        assert kvsep.combine(c, 0, 0) == c


def test_associative_over_three_parts(oracle):
    data = splitmix64_bytes(70000, 7, 0)
    base = data.ctypes.data
    for la, lb, lc in ((0, 0, 0), (1, 1, 1), (17, 4097, 255), (4096, 0, 65535 - 4096), (3, 60000, 16), (0, 5, 0)):
        va = oracle.extend_addr(0, base, la)
        vb = oracle.extend_addr(0, base + la, lb)
        vc = oracle.extend_addr(0, base + la + lb, lc)
        left = kvsep.combine(kvsep.combine(va, vb, lb), vc, lc)
        right = kvsep.combine(va, kvsep.combine(vb, vc, lc), lb + lc)
        assert left == right == oracle.extend_addr(0, base, la + lb + lc), (la, lb, lc)
        for init in (0x12345678, 0xFFFFFFFF):  # ... and on top of an init
            assert kvsep.combine(init, left, la + lb + lc) == oracle.extend_addr(init, base, la + lb + lc)


# ---------------------------------------------------------------- the independent computation
POLY = 0x11EDC6F41  # x^32 + ... + 1, Castagnoli, bit i = coefficient of x^i


def _rev32(v):
    return int(f"{v:032b}"[::-1], 2)


def _polymulmod(a, b):
    """a * b mod POLY over GF(2), bit by bit."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 32:
            a ^= POLY
    return r


def _x_to(e):
    """x^e mod POLY, e any Python integer >= 0."""
    r, sq = 1, 2
    while e:
        if e & 1:
            r = _polymulmod(r, sq)
        sq = _polymulmod(sq, sq)
        e >>= 1
    return r


def _shift(c, n):
    """c * x^(8n) mod P for a CRC value c in the library's reflected representation (bit 31 = x^0)."""
    return _rev32(_polymulmod(_rev32(c), _x_to(8 * n)))


@pytest.mark.parametrize("n", [0, 1, 4096, 2**32 + 77, 2**40, 2**61 - 1, 2**61, 2**61 + 1, 2**63, 2**64 - 1])
def test_combine_is_the_polynomial_shift_for_every_64_bit_length(n):
    for c in (0, 1, 0x80000000, 0x82F63B78, 0xDEADBEEF, 0xFFFFFFFF, 0x12345678):
        assert kvsep.combine(c, 0, n) == _shift(c, n), (hex(c), n)
        assert kvsep.combine(c, 0xA5A5A5A5, n) == _shift(c, n) ^ 0xA5A5A5A5


def test_python_shift_agrees_with_the_oracle_on_real_zero_bytes(oracle):
    """The plain-Python arithmetic above is itself checked: advancing over n zero bytes is the shift."""
    z = np.zeros(5000, np.uint8)
    for n in (0, 1, 4, 255, 4999):
        for c in (0x12345678, 0xFFFFFFFF):
            # Extend(c, zeros) = c * X(n) ^ Value(zeros)
            assert oracle.extend_addr(c, z.ctypes.data, n) == _shift(c, n) ^ oracle.extend_addr(0, z.ctypes.data, n)
