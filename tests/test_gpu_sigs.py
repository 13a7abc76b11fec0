"""GPU: signatures verified in place from per-signature descriptors (fdgpu_ed25519_verify_sigs_device / _host,
DESIGN 21: fd_sig_size_kernel, fd_sig_scan_kernel, fd_sig_place_kernel, fd_sig_pack_kernel, fd_sig_flag_kernel in
front of and behind an unchanged batch).

Every expected code is the CPU oracle's fd_ed25519_verify of the triple a descriptor names, or FDGPU_ERR_DESC for a
bad descriptor.  A valid signature verifies only if every one of its 96 + msg_sz bytes reached the pack arena
unchanged and the padding behind it did not leak into the message, so the codes check the copy itself.

test_parity_on_every_engine_path runs under the suite's engine-path parameter (tests/conftest.py).  The other
scenarios choose their options themselves, so they run on the GPU once (_once) and the suite's repeats only find
that they passed.
"""
import functools
import hashlib

import numpy as np
import pytest

from firedancer_amd import engine
from tests import test_gpu_key_split as ks

pytestmark = pytest.mark.gpu

ERR = engine.FDGPU_ERR_DESC
SLACK = engine.ARENA_SLACK
SIZES = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1167, 1232, 4095, 4096,
         65439)
COUNTS = (1, 63, 64, 65, 255, 256, 257)


def _once(f):
    return functools.lru_cache(maxsize=None)(f)


def _msg(t, n):
    return hashlib.shake_256(b"sigs %d" % t).digest(n) if n else b""


def _triple(key, t, n):
    """(sig, pub, msg): message number t of n bytes, signed by key number key"""
    m = _msg(t, n)
    sig, pub = ks._sign(key, m)
    return sig, pub, m


def _tamper(tr, kind, other_pub):
    sig, pub, m = tr
    if kind == 0 and m:
        m = m[:len(m) // 2] + bytes([m[len(m) // 2] ^ 0x20]) + m[len(m) // 2 + 1:]
    elif kind == 1 or kind == 0:
        sig = sig[:32] + bytes(32)
    else:
        pub = other_pub
    return sig, pub, m


def _want(triples, sem=0):
    o = ks._oracle()
    return np.array([o.verify(m, s, p, sem) for s, p, m in triples], np.int8)


class _Arena:
    """Bytes laid end to end, each piece at a chosen offset mod 16 behind a gap of junk"""

    def __init__(self, seed):
        self.b = bytearray()
        self.rng = np.random.default_rng(seed)

    def put(self, data, mod=None):
        if mod is None:
            mod = int(self.rng.integers(0, 16))
        gap = (mod - len(self.b)) % 16
        self.b += self.rng.integers(1, 256, gap, dtype=np.uint8).tobytes()     # (never zero: a leak shows)
        off = len(self.b)
        self.b += data
        return off

    def array(self):
        """(the arena page-aligned with its slack behind it, arena_sz)"""
        n = len(self.b)
        raw = np.zeros(n + SLACK + 8192, np.uint8)
        o = (-raw.ctypes.data) % 4096
        a = raw[o:o + n + SLACK]
        a[:n] = np.frombuffer(bytes(self.b), np.uint8)
        a[n:] = 0xEE
        return a, n


def _scatter(triples, seed):
    """An arena holding every triple's three parts at random alignments, in shuffled order, and the descriptors"""
    ar = _Arena(seed)
    desc = np.zeros(len(triples), engine.SIG_DESC_DTYPE)
    parts = [(i, j) for i in range(len(triples)) for j in range(3)]
    ar.rng.shuffle(parts)
    for i, j in parts:
        desc[i][("sig_off", "pub_off", "msg_off")[j]] = ar.put(triples[i][j])
    desc["msg_sz"] = [len(t[2]) for t in triples]
    a, n = ar.array()
    return a, n, desc


def _bound(desc):
    """104 cnt + msg_bytes: what a batch needs at most"""
    return 104 * len(desc) + int(desc["msg_sz"].astype(np.int64).sum())


def _device(eng, arena, arena_sz, desc, msg_bytes=None):
    import torch
    a = torch.from_numpy(arena).cuda()
    d = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8)).cuda()
    out = torch.full((len(desc),), 7, dtype=torch.int8, device="cuda")
    if msg_bytes is None:
        msg_bytes = int(desc["msg_sz"].astype(np.int64).sum())
    eng.verify_sigs_device(a.data_ptr(), arena_sz, d.data_ptr(), len(desc), msg_bytes, out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _registered(eng, arena, arena_sz, desc):
    engine.host_register(arena)
    try:
        return eng.verify_sigs_host(arena, desc, arena_sz)
    finally:
        engine.host_unregister(arena)


def _plain(eng, arena, arena_sz, desc):
    return eng.verify_sigs_host(arena.copy(), desc, arena_sz)


def _all_forms(eng, arena, arena_sz, desc, want, what, msg_bytes=None):
    np.testing.assert_array_equal(_device(eng, arena, arena_sz, desc, msg_bytes), want, err_msg=str((what, "device")))
    for name, f in (("registered", _registered), ("plain", _plain)):
        np.testing.assert_array_equal(f(eng, arena, arena_sz, desc), want, err_msg=str((what, name)))


def _engine(n, payload=0, prepare=None, defaults=True, **opts):
    import firedancer_amd as fa
    fa.load_library()
    if defaults:
        engine.debug_reset_opts()
    if opts:
        engine.debug_set_opts(**opts)
    try:
        eng = fa.Engine(device=0, max_txn=n, max_sig=n, max_payload=payload)
    finally:
        if opts:
            engine.debug_reset_opts()
    if prepare:
        eng.sigs_prepare(prepare)
    return eng


def _refused(f, *a):
    with pytest.raises(RuntimeError) as e:
        f(*a)
    return e.value.args[1]


# ---- 1: parity on every engine path ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _parity_batch():
    rng = np.random.default_rng(20261020)
    triples = []
    for t in range(300):
        tr = _triple(t % 32, t, int(rng.integers(0, 1233)))
        if t % 5 == 2:
            tr = _tamper(tr, (t // 5) % 3, ks._key((t + 1) % 32)[0])
        triples.append(tr)
    return _scatter(triples, 1) + (_want(triples),)


def test_parity_on_every_engine_path(engine_path):
    arena, arena_sz, desc, want = _parity_batch()
    assert (want != 0).sum() == 60 and (want == 0).sum() == 240
    eng = _engine(300, payload=300 * 1400, prepare=_bound(desc), defaults=False)
    try:
        _all_forms(eng, arena, arena_sz, desc, want, engine_path)
    finally:
        eng.close()


# ---- 2: copy edges ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _edge_batch():
    ar = _Arena(2)
    triples, rows = [], []

    def add(tr, s, p, m):
        triples.append(tr)
        rows.append((s, p, m, len(tr[2])))

    for t, n in enumerate(SIZES):                            # every message size, parts at random alignments
        tr = _triple(t % 7, 1000 + t, n)
        add(tr, ar.put(tr[0]), ar.put(tr[1]), ar.put(tr[2]))
    base = _triple(3, 2000, 100)                              # one 100-byte message: each offset mod 16, one at a time
    for part in range(3):
        for v in range(16):
            mods = [5, 9, 14]
            mods[part] = v
            add(base, ar.put(base[0], mods[0]), ar.put(base[1], mods[1]), ar.put(base[2], mods[2]))
    for v in range(16):                                       # ... and all three moving
        add(base, ar.put(base[0], v), ar.put(base[1], (5 * v + 3) % 16), ar.put(base[2], (11 * v + 7) % 16))
    # the prune shape: two descriptors share the signature and the key, the messages differ
    a, b = _triple(4, 2100, 77), _triple(4, 2101, 77)
    s, p = ar.put(a[0]), ar.put(a[1])
    add(a, s, p, ar.put(a[2]))
    add((a[0], a[1], b[2]), s, p, ar.put(b[2]))
    # a message range that holds its own signature (and the key's first bytes)
    c = _triple(5, 2102, 40)
    s = ar.put(c[0] + c[1])
    at = len(ar.b)
    whole = bytes(ar.b[s - 30: at])
    add((c[0], c[1], whole), s, s + 64, s - 30)
    while len(triples) < max(COUNTS) - 1:                     # ordinary records up to the largest count
        t = len(triples)
        tr = _triple(t % 11, 3000 + t, (t * 37) % 301)
        if t % 6 == 0:
            tr = _tamper(tr, t % 3, ks._key(40)[0])
        add(tr, ar.put(tr[0]), ar.put(tr[1]), ar.put(tr[2]))
    last = _triple(6, 2103, 133)                              # its message ends exactly at arena_sz
    add(last, ar.put(last[0]), ar.put(last[1]), ar.put(last[2], 3))
    arena, arena_sz = ar.array()
    desc = np.array(rows, engine.SIG_DESC_DTYPE)
    assert int(desc["msg_off"][-1]) + int(desc["msg_sz"][-1]) == arena_sz and len(desc) == max(COUNTS)
    return arena, arena_sz, desc, _want(triples)


@_once
def _copy_edges():
    arena, arena_sz, desc, want = _edge_batch()
    assert (want[:len(SIZES)] == 0).all() and (want[len(SIZES):len(SIZES) + 64] == 0).all() and want[-1] == 0
    eng = _engine(len(desc), payload=1 << 20, prepare=_bound(desc))
    try:
        _all_forms(eng, arena, arena_sz, desc, want, "all")
        for cnt in COUNTS:
            # the last record, whose message ends the arena, closes every count
            d = np.concatenate([desc[:cnt - 1], desc[-1:]])
            w = np.concatenate([want[:cnt - 1], want[-1:]])
            np.testing.assert_array_equal(_device(eng, arena, arena_sz, d), w, err_msg=str(cnt))
            np.testing.assert_array_equal(_registered(eng, arena, arena_sz, d), w, err_msg=str(cnt))
    finally:
        eng.close()


def test_copy_edges():
    """Every message size around a dword, a store and a turn of the copy loop; every alignment of each part; the
    arena's last byte; overlapping ranges; record counts around a wavefront and a block"""
    _copy_edges()


# ---- 3: the scan across both levels -------------------------------------------------------------------------

@_once
def _scan_levels():
    n = 70001
    triples = []
    for t in range(300):
        tr = _triple(t % 32, 5000 + t, t % 9)
        if t % 5 == 1:
            tr = _tamper(tr, (t // 5) % 3, ks._key((t + 3) % 32)[0])
        triples.append(tr)
    arena, arena_sz, d300 = _scatter(triples, 3)
    w300 = _want(triples)
    idx = (np.arange(n, dtype=np.int64) * 7919 + 13) % 300
    desc, want = d300[idx], w300[idx]
    eng = _engine(n, prepare=_bound(desc))
    try:
        got = _device(eng, arena, arena_sz, desc)
        for i in (0, 255, 256, 65535, 65536, n - 1):
            assert got[i] == want[i], (i, got[i], want[i])
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(_registered(eng, arena, arena_sz, desc), want)
    finally:
        eng.close()


def test_scan_across_both_levels():
    """70,001 descriptors over 300 triples: 274 blocks of 256, so the block totals take two turns of the second
    level; default options send the batch down the throughput path"""
    _scan_levels()


# ---- 4: bad descriptors -------------------------------------------------------------------------------------

@_once
def _bad_descriptors():
    triples = [_triple(t % 5, 6000 + t, 20 + 13 * t) for t in range(8)]
    triples[3] = _tamper(triples[3], 0, None)
    ar = _Arena(4)
    ar.put(bytes(70000))                                      # so that msg_sz = 65,440 at offset 0 is inside the arena
    good = [(ar.put(s), ar.put(p), ar.put(m), len(m)) for s, p, m in triples]
    arena, A = ar.array()
    g = good[0]
    bad = [(A - 63, g[1], g[2], g[3]), (g[0], A - 31, g[2], g[3]), (g[0], g[1], A - g[3] + 1, g[3]),
           (0xFFFFFFF0, g[1], g[2], g[3]), (g[0], g[1], 0xFFFFFFFF, 2), (g[0], g[1], 0, 65440),
           (g[0], g[1], g[2], 0xFFFFFFFF)]
    rows, want, w8 = [], [], _want(triples)
    for i in range(8):
        rows.append(good[i])
        want.append(w8[i])
        if i < len(bad):
            rows.append(bad[i])
            want.append(ERR)
    desc, want = np.array(rows, engine.SIG_DESC_DTYPE), np.array(want, np.int8)
    assert (want == ERR).sum() == 7 and want[0] == 0 and want[-1] == 0 and want[6] == -3
    # each field one byte less is good: the bad ones above are past the end by exactly one byte
    edge = np.array([(A - 64, g[1], g[2], g[3]), (g[0], A - 32, g[2], g[3]), (g[0], g[1], A - g[3], g[3])],
                    engine.SIG_DESC_DTYPE)
    # msg_bytes is the caller's sum over the records it means to verify; the device trusts none of it
    honest = sum(r[3] for r in good)
    eng = _engine(len(desc), payload=1 << 20, prepare=104 * len(desc) + honest)
    try:
        _all_forms(eng, arena, A, desc, want, "bad", honest)
        _all_forms(eng, arena, A, desc[1:2], want[1:2], "a bad one alone", 0)
        got = _device(eng, arena, A, edge)
        assert (got != ERR).all() and np.isin(got, (0, -1, -2, -3)).all(), got
        np.testing.assert_array_equal(_plain(eng, arena, A, edge), got)
    finally:
        eng.close()


def test_bad_descriptors():
    """Each bad descriptor between two good records, which keep their codes; all three forms agree"""
    _bad_descriptors()


# ---- 5: capacity and refusals -------------------------------------------------------------------------------

@_once
def _capacity():
    n, k = 40, 17
    triples = [_triple(t % 6, 7000 + t, 300 + (t * 53) % 900) for t in range(n)]
    triples[9] = _tamper(triples[9], 2, ks._key(50)[0])
    arena, A, desc = _scatter(triples, 5)
    want = _want(triples)
    desc[5]["pub_off"] = A - 31                               # a bad record inside the part that fits: 96 bytes
    want[5] = ERR
    size = np.where(np.arange(n) == 5, 96, (96 + desc["msg_sz"].astype(np.int64) + 7) // 8 * 8)
    cap = int(size[:k].sum())
    assert 104 * n <= cap
    eng = _engine(n, payload=1 << 20)
    try:
        # unprepared
        assert _refused(_device, eng, arena, A, desc) == -3
        assert _refused(_registered, eng, arena, A, desc) == -3
        eng.sigs_prepare(cap)
        # an understated msg_bytes: the device places the records itself
        got = _device(eng, arena, A, desc, msg_bytes=0)
        np.testing.assert_array_equal(got[:k], want[:k])
        assert (got[k:] == ERR).all(), got
        # one byte less: record k - 1 no longer fits
        eng2 = _engine(n, prepare=cap - 1)
        try:
            got = _device(eng2, arena, A, desc, msg_bytes=0)
            np.testing.assert_array_equal(got[:k - 1], want[:k - 1])
            assert (got[k - 1:] == ERR).all(), got
        finally:
            eng2.close()
        # the honest sum is refused, and so are too many records
        assert _refused(_device, eng, arena, A, desc) == -1
        eng.sigs_prepare(1 << 20)
        big = np.concatenate([desc, desc])
        assert _refused(_device, eng, arena, A, big) == -1
        # correctly sized, the same context returns the oracle's codes; the host form cuts chunks that fit
        np.testing.assert_array_equal(_device(eng, arena, A, desc), want)
        np.testing.assert_array_equal(_registered(eng, arena, A, big), np.concatenate([want, want]))
        # a smaller size changes nothing
        eng.sigs_prepare(cap)
        np.testing.assert_array_equal(_device(eng, arena, A, desc), want)
        # the async pipeline holds a transaction: the synchronous calls' refusal
        sig, pub, m = triples[0]
        assert eng.submit(sig + pub + m, 0, 64, 96, 1, 7) == 0
        assert _refused(_registered, eng, arena, A, desc) == -1
        assert _refused(_plain, eng, arena, A, desc) == -1
        with pytest.raises(RuntimeError):
            eng.verify_many([m], [sig], [pub])
        eng.flush()
        tags, codes = eng.poll(blocking=True)
        assert list(tags) == [7] and list(codes) == [0]
        np.testing.assert_array_equal(_registered(eng, arena, A, desc), want)
        # a faulted context
        eng.debug_fault()
        assert _refused(_device, eng, arena, A, desc) == -3
    finally:
        eng.close()
    # the host form over a registered region in chunks: a prepared size that holds a few records at a time
    eng = _engine(n, prepare=4000)
    try:
        np.testing.assert_array_equal(_registered(eng, arena, A, desc), want)
    finally:
        eng.close()


def test_capacity_and_refusals():
    _capacity()


# ---- 6: pins reach these callers ----------------------------------------------------------------------------

@_once
def _pins():
    keys = []
    for c in range(40):                                       # 40 cold keys, one record each, among 4 x 15 pinned
        keys.append(100 + c)
        keys += [(3 * c + j) % 4 for j in range(3)] if c < 20 else []
    assert len(keys) == 100 and all(keys.count(p) == 15 for p in range(4))
    triples = [_triple(kk, 8000 + i, 40 + (i * 29) % 500) for i, kk in enumerate(keys)]
    triples[0] = _tamper(triples[0], 0, None)
    arena, A, desc = _scatter(triples, 6)
    want = _want(triples)
    eng = _engine(4096, prepare=_bound(desc), half=1, small_batch_max=0)
    try:
        assert eng.pin_cap() == 24
        eng.set_pinned_keys([ks._key(p)[0] for p in range(4)])
        np.testing.assert_array_equal(_device(eng, arena, A, desc), want)
        assert eng.pinned_count() == (4, 60), eng.pinned_count()
    finally:
        eng.close()


def test_pins_reach_these_callers():
    _pins()
