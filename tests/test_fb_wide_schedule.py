"""The wide fixed-base walk's schedule and digit split (fd_fb_wide_* in firedancer_amd/csrc/fd_gpu_lattice.h), compiled
as host C: the same index arithmetic the body dsmf_wide of fd_dsmh_kernel and the builds of fd_ftab_kernel use
(DESIGN 20).

Span t of k is v_t = sum_{r<4} a_(4t+r) 2^(8r) over fd_fb_recode's byte digits, split as d0 + 2^11 d1 + 2^22 d2.  A
slot's wide tables are modelled as integers, entry e of table (t, r) as e 2^(32t + 11r), and the base point's as in
tests/test_fb_full_schedule.py.  Driven through the host functions, the 40 additions must recompose k and S, every
digit must fit its table, and the third table's size FD_FB_W2 must be the proven bound on |d2| rounded up to a
multiple of 8.

A wave that holds a full slot without wide tables does not run a per-lane mixture of the two geometries: all its
lanes walk dsmf_full's 48 additions from the byte tables, which a wide slot has too (departures).  The
mixed-wave test pins that down: such a wave's schedule is fd_fb_full_*'s, unchanged."""
import ctypes
import random

import numpy as np
import pytest

from tests.test_fb_full_schedule import _digits_b, _full, _pairs, _walk_full
from tests.test_fb_recode import L, _check

NB = 16
D2_MIN, D2_MAX = -514, 510          # reasoned in fd_gpu_lattice.h; test_digit_bounds finds both by exhaustion


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import build
    return ctypes.CDLL(build.build_lattice_host())


@pytest.fixture(scope="module")
def geom(lib):
    w0, w2, we, wcap = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.fd_fb_wide_geom_host(ctypes.byref(w0), ctypes.byref(w2), ctypes.byref(we), ctypes.byref(wcap))
    return w0.value, w2.value, we.value, wcap.value


def _wide(lib):
    out = (ctypes.c_int * (4 * 40))()
    n = lib.fd_fb_wide_sched_host(out)
    return [tuple(out[4 * i + j] for j in range(4)) for i in range(n)]


def _split(lib, a4):
    return [lib.fd_fb_wide_split_host(a4[0], a4[1], a4[2], a4[3], r) for r in range(3)]


def _model(a0, a1, a2, a3):
    """The split on exact integers (numpy int64 or Python ints): the signed low 11 bits, twice, and what is left"""
    v = a0 + (a1 << 8) + (a2 << 16) + (a3 << 24)
    d0 = ((v + 1024) & 2047) - 1024
    v1 = (v - d0) >> 11
    d1 = ((v1 + 1024) & 2047) - 1024
    return d0, d1, (v1 - d1) >> 11


def _walk_wide(lib, a, b):
    """The 40 additions on integers; every key digit must fit its table"""
    acc = 0
    for base, span, dig, table in _wide(lib):
        if base:
            d = b[dig]
            assert lib.fd_fb_entry_host(d) == abs(d) <= 32768
            acc += d << (16 * table)
        else:
            d = _split(lib, a[4 * span:4 * span + 4])[dig]
            assert table == 3 * span + dig
            assert lib.fd_fb_entry_host(d) == abs(d) <= lib.fd_fb_wide_entries_host(dig), (a[4 * span:4 * span + 4], dig, d)
            acc += d << (32 * span + 11 * dig)
    return acc


def test_geometry(lib, geom):
    w0, w2, we, wcap = geom
    assert (w0, we, wcap) == (1024, 2 * 1024 + w2, 1024) and w2 % 8 == 0
    assert [lib.fd_fb_wide_entries_host(r) for r in range(3)] == [w0, w0, w2]
    # the 24 tables of a key's row are laid end to end
    end = 0
    for t in range(8):
        for r in range(3):
            assert lib.fd_fb_wide_off_host(t, r) == end
            end += lib.fd_fb_wide_entries_host(r)
    assert end == 8 * we == 20544


def test_wide_walk_recomposes_k_and_s(lib):
    for k, s in _pairs():
        a, b = _check(lib, k), _digits_b(s)
        assert _walk_wide(lib, a, [0] * 16) == k and _walk_wide(lib, [0] * 32, b) == s, (hex(k), hex(s))
        assert _walk_wide(lib, a, b) == _walk_full(lib, a, b) == k + s


def test_digit_bounds(lib, geom):
    w0, w2, _, _ = geom
    # every span there is: d1 and d2 depend on a0, a1 only through (v - d0) >> 11, so all (a0, a1) give the carries
    # and all (carry, a2, a3) the digits
    a0, a1 = np.meshgrid(np.arange(-128, 128, dtype=np.int64), np.arange(-128, 128, dtype=np.int64), indexing="ij")
    d0 = ((a0 + 256 * a1 + 1024) & 2047) - 1024
    assert d0.min() == -1024 and d0.max() == 1023
    carry = (a0 + 256 * a1 - d0) >> 11
    carries = np.unique(carry)
    c, a2, a3 = np.meshgrid(carries, np.arange(-128, 128, dtype=np.int64), np.arange(-128, 128, dtype=np.int64), indexing="ij")
    v1 = c + 32 * a2 + 8192 * a3
    d1 = ((v1 + 1024) & 2047) - 1024
    d2 = (v1 - d1) >> 11
    assert d1.min() == -1024 and d1.max() == 1023
    assert (int(d2.min()), int(d2.max())) == (D2_MIN, D2_MAX)
    big = max(-D2_MIN, D2_MAX)
    assert big <= w2 <= big + 8

    # the C function on the spans at the ends: all -128, all 127, and the mixed-sign spans with the same d2
    ends = [[-128] * 4, [127] * 4]
    for want in (D2_MIN, D2_MAX):
        ic, i2, i3 = (x[:6] for x in np.nonzero(d2 == want))
        for jc, j2, j3 in zip(ic, i2, i3):
            # low bytes of opposite signs that carry the same into v1
            i0, i1 = (x[0] for x in np.nonzero((carry == carries[jc]) & ((a0 < 0) != (a1 < 0))))
            ends.append([int(i0) - 128, int(i1) - 128, int(j2) - 128, int(j3) - 128])
    assert any(min(a) < 0 <= max(a) for a in ends)
    seen = set()
    for a in ends:
        d = _split(lib, a)
        assert tuple(d) == tuple(int(x) for x in _model(*a)), a
        assert -w0 <= d[0] < w0 and -w0 <= d[1] < w0 and abs(d[2]) <= w2, (a, d)
        assert d[0] + (d[1] << 11) + (d[2] << 22) == sum(x << (8 * r) for r, x in enumerate(a))
        seen.add(d[2])
    assert {D2_MIN, D2_MAX} <= seen
    assert _split(lib, [-128] * 4)[2] == D2_MIN and _split(lib, [127] * 4)[2] == D2_MAX

    # random spans against the model, and the top span of k = l - 1
    rng = random.Random(20)
    for _ in range(20000):
        a = [rng.randrange(-128, 128) for _ in range(4)]
        assert tuple(_split(lib, a)) == tuple(_model(*a)), a
    top = _check(lib, L - 1)[28:]
    assert top == [0, 0, 0, 0x10] and _split(lib, top) == [0, 0, 64]


def test_wide_schedule_shape(lib):
    sched = _wide(lib)
    assert len(sched) == 40 == lib.fd_fb_wave_adds_host(1)
    assert sorted(t for base, _, _, t in sched if not base) == list(range(24))      # every wide table exactly once
    assert sorted(t for base, _, _, t in sched if base) == list(range(NB))
    assert [base for base, _, _, _ in sched] == [0, 0, 0, 1, 1] * 8                   # per span: the key's three, then B's two
    assert [span for _, span, _, _ in sched] == [i // 5 for i in range(40)]
    for base, span, dig, table in sched:
        assert (dig == table and table in (2 * span, 2 * span + 1)) if base else (table == 3 * span + dig and 0 <= dig < 3)


def test_mixed_wave_walks_the_byte_schedule(lib):
    """A wave with one full slot that has no wide tables: 48 additions, and every lane -- of either kind of slot --
    reads exactly fd_fb_full_*'s schedule, so only the byte tables and the base point's, none of the wide ones"""
    full = _full(lib)
    assert lib.fd_fb_wave_adds_host(0) == 48 == len(full)
    assert sorted(t for base, _, t in full if not base) == list(range(32))
    # the 8 additions past the wide walk's 40 are the byte schedule's own tail
    assert full[40:] == [(0, 27, 27), (1, 13, 13), (0, 28, 28), (0, 29, 29), (1, 14, 14), (0, 30, 30), (0, 31, 31), (1, 15, 15)]
