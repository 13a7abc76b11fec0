"""The skewed pair for signatures of a repeated key (fd_lat_skew in firedancer_amd/csrc/fd_gpu_lattice.h), the
device reduction compiled as host C.

Q = [c1 S mod l]B + sum_p [c0_p]([2^(68 p)](-A)) + [c1](-R) == O is the reference's verdict exactly when
c0 = sum_p 2^(68 p) c0_p == c1 k (mod 8l) and c1 is odd with 0 < |c1| < l.  Every pair returned must
satisfy that and the stored bounds: nwin <= 20 windows, c0 < 2^(4 (34 + nwin) - 1), |c1| < 2^(4 nwin - 1)
(DESIGN 15).  No hash-distributed k may fail, and at most 0.5 % of them may need more than 17 windows."""
import collections
import ctypes
import os

import numpy as np
import pytest

L = 2**252 + 27742317777372353535851937790883648493
N8L = 8 * L
W, NW = 17, 20
N_RANDOM = 10**6


@pytest.fixture(scope="module")
def lat():
    from firedancer_amd import build
    lib = ctypes.CDLL(build.build_lattice_host())
    lib.fd_lat_skew_host_many.restype = None
    lib.fd_lat_skew_host_many.argtypes = [ctypes.c_ulong] + [ctypes.c_void_p] * 6
    return lib


def _run(lib, ks):
    """[(ok, c0, c1, nwin)] for the scalars ks, through one call."""
    n = len(ks)
    kb = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks), np.uint32).copy()
    c0, c1 = np.zeros(7 * n, np.uint32), np.zeros(5 * n, np.uint32)
    neg, nwin, ok = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.fd_lat_skew_host_many(n, kb.ctypes.data, c0.ctypes.data, c1.ctypes.data, neg.ctypes.data, nwin.ctypes.data,
                              ok.ctypes.data)
    b0, b1 = c0.tobytes(), c1.tobytes()
    out = []
    for i in range(n):
        v1 = int.from_bytes(b1[20 * i: 20 * i + 20], "little")
        out.append((int(ok[i]), int.from_bytes(b0[28 * i: 28 * i + 28], "little"), -v1 if neg[i] else v1, int(nwin[i])))
    return out


def _check(k, c0, c1, nwin):
    assert (c0 - c1 * k) % N8L == 0, hex(k)
    assert c1 % 2 == 1 and 0 < abs(c1) < L, hex(k)
    assert 1 <= nwin <= NW, (hex(k), nwin)
    assert 0 <= c0 < 2**(4 * (2 * W + nwin) - 1) and abs(c1) < 2**(4 * nwin - 1), (hex(k), nwin)


def test_random_k(lat):
    rng = np.random.default_rng(20261019)
    raw = rng.bytes(64 * N_RANDOM)
    ks = [int.from_bytes(raw[64 * i: 64 * i + 64], "little") % L for i in range(N_RANDOM)]     # as SHA-512 mod l
    hist, fails = collections.Counter(), 0
    for k, (ok, c0, c1, nwin) in zip(ks, _run(lat, ks)):
        if not ok:
            fails += 1
            continue
        _check(k, c0, c1, nwin)
        hist[nwin] += 1
    print("windows histogram:", sorted(hist.items()), "failed:", fails)
    assert fails == 0, fails
    over = sum(c for w, c in hist.items() if w > W)
    assert over <= N_RANDOM // 200, (over, sorted(hist.items()))


EDGE = [0, 1, 2, L - 1, L - 2, 2**252] + [N8L // j + d for j in range(9, 41) for d in (-1, 1)]


def test_edge_k(lat):
    assert all(0 <= k < L for k in EDGE)
    res = _run(lat, EDGE)
    for k, (ok, c0, c1, nwin) in zip(EDGE, res):
        if ok:
            _check(k, c0, c1, nwin)
    by_k = dict(zip(EDGE, res))
    assert by_k[0][:3] == (1, 0, -1) or by_k[0][:3] == (1, 0, 1)
    assert by_k[1][0] and by_k[2][0]                     # already short: c1 = +-1
    assert abs(by_k[1][2]) == 1 and abs(by_k[2][2]) == 1
    assert not by_k[L - 1][0]                            # every odd-c1 vector has c0 ~ l: refused, not a long pair
