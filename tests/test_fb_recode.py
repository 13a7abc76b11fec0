"""The fixed-base walk's digits of k (fd_fb_recode in firedancer_amd/csrc/fd_gpu_lattice.h), compiled as host C.

fd_hashh_kernel stores k mod l of a fixed-base signature as 32 signed radix-256 digits, and the walk reads digit
j = 4 t + r as a multiple (at most 128, the table's size) of [2^(32 t)](-A) at bit offset 8 r.  So every digit must
lie in [-128, 128), the digits must recompose to k, and for k < l nothing may be carried out of the top digit.
The last test walks the schedule of fd_dsmh_kernel's fixed-base body on integers instead of points."""
import ctypes
import random

import pytest

L = 2**252 + 27742317777372353535851937790883648493


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import build
    return ctypes.CDLL(build.build_lattice_host())


def _recode(lib, k):
    kw = (ctypes.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
    d = (ctypes.c_byte * 32)()
    carry = lib.fd_fb_recode_host(d, kw)
    return [int(x) for x in d], int(carry)


def _check(lib, k):
    d, carry = _recode(lib, k)
    assert all(-128 <= x < 128 for x in d), (hex(k), d)
    assert sum(x << (8 * j) for j, x in enumerate(d)) + (carry << 256) == k, hex(k)
    if k < L:
        assert carry == 0, hex(k)
    return d


def test_random_k(lib):
    rng = random.Random(20261019)
    for _ in range(20000):
        _check(lib, rng.randrange(L))


def _x80(top):
    """0x80 in every byte below the top one: every digit but the lowest is -127 with a carry"""
    return int.from_bytes(bytes([0x80] * 31 + [top]), "little")


EDGES = [0, 1, 127, 128, 255, 256, L - 1, L - 2, 2**252, 2**252 - 1, 2**128, 2**128 - 1,
         _x80(0x00), _x80(0x0f), _x80(0x10) % L, _x80(0x7e), _x80(0x7f), _x80(0x80), 2**256 - 1,
         int.from_bytes(bytes([0x7f, 0x80] * 16), "little"), int.from_bytes(bytes([0x80, 0x7f] * 16), "little"),
         int.from_bytes(bytes([0xff] * 31 + [0x0f]), "little")]


@pytest.mark.parametrize("k", EDGES)
def test_edge_k(lib, k):
    d = _check(lib, k)
    if k == 0:
        assert d == [0] * 32
    if k == _x80(0x80):
        assert d == [-128] + [-127] * 31 and _recode(lib, k)[1] == 1


def test_walk_schedule_recomposes(lib):
    """Four steps at bit offsets 24, 16, 8, 0 with 8 doublings between them: the step at offset 8 r adds digit
    a_(4t+r) times 2^(32 t) for t = 0..7, and the steps at offsets 16 and 0 the radix-2^16 digits b_(2t+1), b_(2t)
    of S times 2^(32 t)."""
    rng = random.Random(7)
    for _ in range(200):
        k, s = rng.randrange(L), rng.randrange(L)
        a = _check(lib, k)
        b, carry = [], 0
        for i in range(16):                      # store_digits_B
            v = ((s >> (16 * i)) & 0xffff) + carry
            carry = (v + 32768) >> 16
            b.append(v - (carry << 16))
        assert carry == 0 and all(abs(x) <= 32768 for x in b)
        acc_a = acc_b = 0
        for r in (3, 2, 1, 0):
            acc_a += sum(a[4 * t + r] << (32 * t) for t in range(8))
            if r % 2 == 0:
                acc_b += sum(b[2 * t + (r >> 1)] << (32 * t) for t in range(8))
            if r:
                acc_a <<= 8
                acc_b <<= 8
        assert acc_a == k and acc_b == s
