"""GPU: a public key with many signatures in a batch gets fixed-base tables of its own and its signatures walk
24 doublings, R compared undecoded (fd_keyclass_kernel, fd_ftab_kernel, the fixed-base body of fd_dsmh_kernel and
the R-check kernels over the fixed-base segment).

Every case runs on small batches forced onto the throughput path (small_batch_max = 0), in both result-code
semantics, with fdgpu_debug_opts_t.key_fixed 0 (on: fixed-base from FD_FB_MIN signatures), 1 (off: the kernels
and launches without it) and 2 (tests: fixed-base from 4 signatures, with key_split = 2 so that keys of 2 and 3
signatures are hot), and with the tables on also through the carry-folded kernels the large batches use
(nofold_max = 0).  The transaction and per-signature codes equal the CPU oracle's in every mode, and the device's
counts of fixed-base and of repeated keys and signatures are the batch's own, so the path cannot be silently off.
The batch helpers are tests/test_gpu_key_split.py's.
"""
import collections
import functools

import numpy as np
import pytest

from tests import test_gpu_key_split as ks

pytestmark = pytest.mark.gpu

ON, OFF, TESTS = 0, 1, 2
FB_MIN = {ON: 128, TESTS: 4}         # FD_FB_MIN, and fdgpu_debug_opts_t.key_fixed = 2
HOT_MIN = {ON: 8, OFF: 8, TESTS: 2}  # key_split rides along: 0, 0, 2
FB_CAP = 4096                        # FD_FB_CAP
L = ks.L
MODES = [(ON, False), (ON, True), (OFF, False), (TESTS, False), (TESTS, True)]


def _engine(fa, n_txn, nsig, nbytes, sem, mode, fold=False):
    from firedancer_amd import engine
    engine.debug_set_opts(half=1, small_batch_max=0, key_fixed=mode, key_split=2 if mode == TESTS else 0,
                          nofold_max=0 if fold else -1)
    try:
        return fa.Engine(device=0, max_txn=n_txn, max_sig=nsig, max_payload=nbytes, semantics=sem)
    finally:
        engine.debug_reset_opts()


@functools.lru_cache(maxsize=None)
def _run(name, sem, mode, fold=False):
    """(txn codes, signature codes, (repeated keys, signatures), (fixed-base keys, signatures)) of one batch on a
    context of its own, run once."""
    import firedancer_amd as fa
    fa.load_library()
    payload, desc, nsig = _batch(name)
    eng = _engine(fa, len(desc), nsig, payload.nbytes, sem, mode, fold)
    try:
        t, s = eng.verify_txns_host(payload, desc)
        return t, s, eng.hot_count(), eng.fixed_count()
    finally:
        eng.close()


def _r_variants():
    """R encodings that are not a valid signature's: non-canonical (y = p + 1, which is also the identity's y),
    undecodable, small order (order 8)"""
    noncanon = (2**255 - 19 + 1).to_bytes(32, "little")
    undec, _, _, small8 = ks._edge_keys()
    return noncanon, undec, small8


COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "one_key":            # 1 key x 300 signatures
        txns = ks._single([0] * 300)
    elif name == "counts":           # keys with exactly COUNTS signatures, shuffled
        keys = [10 + i for i, c in enumerate(COUNTS) for _ in range(c)]
        np.random.default_rng(16).shuffle(keys)
        txns = ks._single(keys)
    elif name == "interleaved":      # one key with 300 signatures, three with 34, keys of 3, 2 and 1 between them
        keys = []
        for t in range(600):
            keys.append(0 if t % 2 == 0 else 1 + (t // 6) % 3 if t % 6 == 1 else 5000 + t)
        tail = keys[300:] + [100, 100, 100, 101, 101, 102, 102, 102]
        np.random.default_rng(3).shuffle(tail)
        txns = ks._single(keys[:300] + tail)
    elif name == "multi":            # three signers: a fixed-base, a hot and a cold key inside one transaction
        txns = []
        for t in range(150):
            m = ks._msg(t, 64)
            tri = [ks._sign(0, m), ks._sign(1 + t % 5, m), ks._sign(3000 + t, m)]
            txns.append((m, [tri[(i + t) % 3] for i in range(3)]))
    elif name in ("edge255", "edge256", "edge257"):   # the fixed-base segment ends at, before and behind a block edge
        txns = ks._single([0] * int(name[4:]) + list(range(7000, 7010)))
    elif name == "bad_sigs":         # under a fixed-base key
        noncanon, undec, small8 = _r_variants()
        txns = []
        for t in range(176):
            m = ks._msg(t)
            sig, pub = ks._sign(7, m)
            sig = bytearray(sig)
            v = t % 11
            if v == 1:
                sig[40] ^= 1                                     # S changed, still below l
            elif v == 2:
                sig[32:] = (L + t).to_bytes(32, "little")        # S >= l
            elif v == 3:
                m = m[:-1] + bytes([m[-1] ^ 0x80])               # another message
            elif v == 4:
                sig[3] ^= 0x10                                   # R corrupted
            elif v == 5:
                sig[:32] = noncanon
            elif v == 6:
                sig[:32] = undec
            elif v == 7:
                sig[:32] = small8
            txns.append((m, [(bytes(sig), pub)]))
    elif name == "bad_keys":         # an undecodable, an x = 0 with sign and two small-order keys, 130 signatures each
        noncanon, undec, small8 = _r_variants()
        txns = []
        for t in range(5 * 130):
            m = ks._msg(t)
            sig = bytearray(ks._sign(1, m)[0])
            if t % 13 == 5:
                sig[:32] = undec                                 # check (3) before (4): R's decode picks the code
            elif t % 13 == 7:
                sig[:32] = small8
            pub = ks._key(1)[0] if t % 5 == 4 else ks._edge_keys()[t % 5]
            txns.append((m, [(bytes(sig), pub)]))
    elif name == "torsion":
        txns = ks._torsion_txns()[0]
    elif name == "hs_top":           # k and S with top digits that carry
        txns = ks._hs_top_txns()
    elif name == "malformed":        # transactions that fail the bounds check among fixed-base signatures
        p, d, n = ks._pack(ks._single([t % 2 for t in range(400)]))
        d = d.copy()
        for t in range(2, 400, 5):
            d["payload_sz"][t] = (int(d["acct_addr_off"][t]) + 31, int(d["message_off"][t]) - 1)[t & 1]
        return p, d, n
    elif name == "no_repeat":        # every key once
        txns = ks._single(range(2000, 2300))
    elif name == "hot_only":         # thirty keys, 10 signatures each
        txns = ks._single([t % 30 for t in range(300)])
    elif name == "cap":              # more fixed-base keys (of 4 signatures) than FD_FB_CAP: the surplus stays hot
        txns = ks._single([t % (FB_CAP + 4) for t in range(4 * (FB_CAP + 4))])
    else:
        raise KeyError(name)
    return ks._pack(txns)


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    p, d, n = _batch(name)
    return ks._oracle().verify_txns(p, d, n, sem=sem, threads=ks.THREADS)


@functools.lru_cache(maxsize=None)
def _repeated(name, bound):
    """(keys, signatures) of the batch's keys of well-formed transactions with >= bound signatures"""
    p, d, n = _batch(name)
    keys = collections.Counter()
    for t in range(len(d)):
        c, sz = int(d["sig_cnt"][t]), int(d["payload_sz"][t])
        if (int(d["signature_off"][t]) + 64 * c > sz or int(d["acct_addr_off"][t]) + 32 * c > sz
                or int(d["message_off"][t]) > sz):
            continue
        for j in range(c):
            at = int(d["payload_off"][t]) + int(d["acct_addr_off"][t]) + 32 * j
            keys[p[at: at + 32].tobytes()] += 1
    rep = [c for c in keys.values() if c >= bound]
    return len(rep), sum(rep)


def _counts_ok(name, mode, hot, fixed):
    assert hot == _repeated(name, HOT_MIN[mode]), (name, mode, hot)
    assert fixed == ((0, 0) if mode == OFF else _repeated(name, FB_MIN[mode])), (name, mode, fixed)


CASES = ["one_key", "counts", "interleaved", "multi", "edge255", "edge256", "edge257", "bad_sigs", "bad_keys",
         "torsion", "hs_top", "malformed", "no_repeat", "hot_only"]


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_codes_equal_oracle_in_every_mode(name, sem):
    want = _want(name, sem)
    sigs = []
    for mode, fold in MODES:
        t, s, hot, fixed = _run(name, sem, mode, fold=fold)
        assert np.isin(s, (0, -1, -2, -3)).all(), np.unique(s)          # nothing left in flight (FD_PEND_*)
        ks._check((t, s), want, (mode, fold))
        sigs.append(s)
        _counts_ok(name, mode, hot, fixed)
    for s in sigs[1:]:
        np.testing.assert_array_equal(sigs[0], s)


def test_cases_have_teeth():
    """The fixtures hold what they are named for (CPU only, but they are this module's)."""
    assert _repeated("one_key", 128) == (1, 300)
    assert _repeated("counts", 128) == (2, 257) and _repeated("counts", 4) == (8, 585)
    assert _repeated("counts", 8) == (6, 576) and _repeated("counts", 2) == (10, 590)
    assert _repeated("interleaved", 128) == (1, 300) and _repeated("interleaved", 8)[0] == 4
    assert _repeated("interleaved", 4)[0] == 4 and _repeated("interleaved", 2)[0] == 7
    assert _repeated("multi", 128) == (1, 150) and _repeated("multi", 8) == (6, 300)
    for n in (255, 256, 257):
        assert _repeated("edge%d" % n, 128) == (1, n)
    assert _repeated("bad_keys", 128) == (5, 650) and _repeated("malformed", 128)[0] == 2
    assert _repeated("torsion", 4) == (4, 40) and _repeated("hs_top", 4)[1] == _batch("hs_top")[2]
    assert _repeated("no_repeat", 2) == (0, 0) and _repeated("hot_only", 8) == (30, 300)
    assert _repeated("hot_only", 128) == (0, 0)
    for sem in (0, 1):
        _, s = _want("bad_sigs", sem)
        v = np.arange(176) % 11
        assert (s[(v == 0) | (v > 7)] == 0).all() and (s[v == 2] == -1).all()
        assert (s[(v == 1) | (v == 3)] == -3).all() and (s[(v >= 4) & (v <= 7)] != 0).all()
        _, s = _want("bad_keys", sem)
        t = np.arange(650)
        assert (s[(t % 5 == 4) & (t % 13 != 5) & (t % 13 != 7)] == 0).all() and (s[t % 5 != 4] != 0).all()
        assert len(np.unique(s[t % 5 == 2])) > 1         # a small-order key: the code depends on R's decode
        assert (_want("hs_top", sem)[1] == 0).all() and (_want("one_key", sem)[1] == 0).all()
    _, s = _want("malformed", 0)
    assert (s[2::5] == -1).all() and (s == 0).sum() > 200


def test_more_keys_than_the_cap():
    """FD_FB_CAP + 4 keys of 4 signatures each on a context that large: FD_FB_CAP of them get tables, the others
    verify as hot keys."""
    want = _want("cap", 0)
    t, s, hot, fixed = _run("cap", 0, TESTS)
    ks._check((t, s), want, "cap")
    assert (s == 0).all()
    assert fixed == (FB_CAP, 4 * FB_CAP) and hot == (FB_CAP + 4, 4 * (FB_CAP + 4))


@pytest.mark.parametrize("mode", [ON, TESTS])
def test_one_context_alternating_batches(fa_mod, mode):
    """One context; batches with fixed-base keys, with hot keys only, of distinct keys and -- after a batch of
    distinct keys -- batches that the de-duplication only samples (no hot and no fixed-base key then): tables,
    counters and the order of the batch before must not show."""
    names = ("one_key", "hot_only", "no_repeat", "counts", "bad_keys", "interleaved")
    b = {n: _batch(n) for n in names}
    eng = _engine(fa_mod, 700, 700, max(x[0].nbytes for x in b.values()), 0, mode)
    try:
        # "B": sampled only, because more than 7/8 of the signatures of the batch before were representatives
        seq = (("one_key", "N"), ("hot_only", "N"), ("no_repeat", "N"), ("one_key", "B"), ("one_key", "N"),
               ("counts", "N"), ("no_repeat", "N"), ("no_repeat", "B"), ("interleaved", "B"), ("bad_keys", "N"),
               ("hot_only", "N"), ("interleaved", "N"), ("one_key", "N"))
        for name, how in seq:
            got = eng.verify_txns_host(b[name][0], b[name][1])
            ks._check(got, _want(name, 0), (name, how))
            if how == "B":
                assert eng.hot_count() == (0, 0) and eng.fixed_count() == (0, 0), (name, how)
            else:
                _counts_ok(name, mode, eng.hot_count(), eng.fixed_count())
    finally:
        eng.close()


@pytest.fixture(scope="module")
def fa_mod():
    import firedancer_amd
    firedancer_amd.load_library()
    return firedancer_amd
