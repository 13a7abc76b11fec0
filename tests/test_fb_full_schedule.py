"""The two fixed-base walks' schedules (fd_fb_old_* and fd_fb_full_* in firedancer_amd/csrc/fd_gpu_lattice.h), compiled
as host C: the same index arithmetic the bodies dsmf_one and dsmf_full of fd_dsmh_kernel use.

A slot's tables are modelled as integers, entry e of the key's table j as e 2^(8j) and entry e of the base point's
table u as e 2^(16u).  Driven through the host functions, both bodies must recompose k and S from the digits of
fd_fb_recode and store_digits_B: the body with doublings (four steps, 8 doublings between them) and the body
without (48 additions, no doubling).  The body with doublings may read only the tables every slot has, j = 0
(mod 4) and the base point's even ones; the body without reads every table exactly once, an entry one addition
ahead at a time (the order is what the kernel prefetches by)."""
import ctypes
import random

import pytest

from tests.test_fb_recode import EDGES, L, _check

NT, NB = 32, 16


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import build
    return ctypes.CDLL(build.build_lattice_host())


def _old(lib, r):
    out = (ctypes.c_int * (3 * 16))()
    n = lib.fd_fb_old_sched_host(r, out)
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n)]


def _full(lib):
    out = (ctypes.c_int * (3 * 48))()
    n = lib.fd_fb_full_sched_host(out)
    return [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n)]


def _digits_b(s):
    """store_digits_B: 16 signed radix-2^16 digits"""
    b, carry = [], 0
    for i in range(16):
        v = ((s >> (16 * i)) & 0xffff) + carry
        carry = (v + 32768) >> 16
        b.append(v - (carry << 16))
    assert carry == 0 and all(abs(x) <= 32768 for x in b)
    return b


def _entry(lib, d, table, base):
    """What an addition contributes: entry |d| of the table, negated for a negative digit"""
    e = lib.fd_fb_entry_host(d)
    assert e == abs(d) and e <= (32768 if base else 128)
    v = e << ((16 if base else 8) * table)
    return -v if d < 0 else v


def _walk_old(lib, a, b):
    acc = 0
    for r in (3, 2, 1, 0):
        for base, dig, table in _old(lib, r):
            acc += _entry(lib, (b if base else a)[dig], table, base)
        if r:
            acc <<= 8
    return acc


def _walk_full(lib, a, b):
    return sum(_entry(lib, (b if base else a)[dig], table, base) for base, dig, table in _full(lib))


def _pairs():
    rng = random.Random(18)
    pairs = [(rng.randrange(L), rng.randrange(L)) for _ in range(200)]
    edges = [k % L for k in EDGES]
    return pairs + [(k, s) for k in edges for s in (0, L - 1)] + [(rng.randrange(L), s) for s in edges]


def test_table_counts(lib):
    nt, nb = ctypes.c_int(), ctypes.c_int()
    lib.fd_fb_tables_host(ctypes.byref(nt), ctypes.byref(nb))
    assert (nt.value, nb.value) == (NT, NB)


def test_both_bodies_recompose_k_and_s(lib):
    for k, s in _pairs():
        a, b = _check(lib, k), _digits_b(s)
        # the two sums are independent: run each walk with the other scalar's digits zeroed
        assert _walk_old(lib, a, [0] * 16) == k and _walk_old(lib, [0] * 32, b) == s, (hex(k), hex(s))
        assert _walk_full(lib, a, [0] * 16) == k and _walk_full(lib, [0] * 32, b) == s, (hex(k), hex(s))
        assert _walk_old(lib, a, b) == _walk_full(lib, a, b) == k + s


def test_old_body_reads_the_tables_every_slot_has(lib):
    """j = 0 (mod 4) of the key's and the even ones of the base point's: a slot that was never promoted holds no other"""
    seen_k, seen_b = set(), set()
    for r in (3, 2, 1, 0):
        sched = _old(lib, r)
        assert len(sched) == (8 if r & 1 else 16)
        for i, (base, dig, table) in enumerate(sched):
            assert base == (i >= 8)
            if base:
                assert table % 2 == 0 and 0 <= table < NB and dig == table + (r >> 1)
                seen_b.add(dig)
            else:
                assert table % 4 == 0 and 0 <= table < NT and dig == table + r
                seen_k.add(dig)
    assert seen_k == set(range(32)) and seen_b == set(range(16))


def test_full_body_reads_every_table_once(lib):
    sched = _full(lib)
    assert len(sched) == 48
    assert sorted(t for base, _, t in sched if not base) == list(range(NT))
    assert sorted(t for base, _, t in sched if base) == list(range(NB))
    assert all(dig == table for _, dig, table in sched)                  # digit j reads table j: no doubling between
    assert [base for base, _, _ in sched] == [0, 0, 1] * 16              # two of the key's, then one of the base point's
