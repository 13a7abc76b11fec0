"""GPU: pinned public keys.  The caller names keys (fdgpu_ed25519_set_pinned_keys); their tables, all 32 per key, are
built at that call and never evicted, and every signature of such a key in a later batch of the half-size
throughput path is fixed-base and walks without doublings, whatever the key's count in the batch (DESIGN 19:
fd_keypin_kernel, the index lanes of fd_keydedup_kernel, fd_keyclass_kernel, fd_keysplit_kernel).

Contexts are made with half = 1 and small_batch_max = 0, and with the product's bounds unless a case says otherwise
(key_fixed = 0: a key is fixed-base by itself from 128 signatures in a batch), so the point of every case is that a
pinned key is fixed-base far below that.  max_sig = 4096 gives 32 slots and a pin cap of 24.  Every case checks the
transaction and per-signature codes against the CPU oracle in both semantics and through both walks (nofold_max -1
and 0) and that no code is left in flight, and compares the device's counts (pinned_count, fixed_count, ffull_count,
fcache_count) with the batch's own composition, which test_fixtures checks on the CPU.  The batch helpers are
tests/test_gpu_key_split.py's, tests/test_gpu_key_fixed.py's and tests/test_gpu_key_cache.py's.

One case differs from its description in the issue: a context of max_sig = 32 cannot take ten_keys' 40 signatures, so
on that context the first batch is eight_c, eight keys that are neither pinned nor in eight_a / eight_b; the
key_cache = 2 context, which has 8 slots at any size, runs ten_keys.
"""
import collections
import functools

import numpy as np
import pytest

from tests import test_gpu_key_cache as kc
from tests import test_gpu_key_split as ks
from tests import torsion

gpu = pytest.mark.gpu          # (per test, not per module: test_fixtures runs without a GPU)

ON, OFF, TESTS = 0, 1, 2
L = ks.L
COMBOS = [(0, False), (0, True), (1, False), (1, True)]      # (semantics, carry-folded kernels)
MAX_SIG = 4096                       # 32 slots at the product's bound of 128, pin cap 24


def _once(f):
    """The suite repeats every GPU test per engine path (tests/conftest.py); this module chooses its engine options
    itself, so a scenario runs on the GPU once and the repeats only find that it passed."""
    return functools.lru_cache(maxsize=None)(f)


def _engine(batches, sem=0, fixed=ON, cache=ON, full=ON, fold=False, max_sig=MAX_SIG, **opts):
    import firedancer_amd as fa
    from firedancer_amd import engine
    fa.load_library()
    o = dict(half=1, small_batch_max=0, key_fixed=fixed, key_split=2 if fixed == TESTS else 0, key_cache=cache,
             key_full=full, nofold_max=0 if fold else -1)
    o.update(opts)
    engine.debug_set_opts(**o)
    try:
        return fa.Engine(device=0, max_txn=max(len(b[1]) for b in batches),
                         max_sig=max_sig or max(b[2] for b in batches),
                         max_payload=max(b[0].nbytes for b in batches), semantics=sem)
    finally:
        engine.debug_reset_opts()


def _pub(i):
    return ks._key(i)[0]


EDGES = (63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "fifteen":            # 300 single-signer transactions, key t % 20: 15 signatures a key
        txns = ks._single([t % 20 for t in range(300)])
    elif name == "one":              # a batch of one signature
        txns = ks._single([3])
    elif name == "five":             # ... and of five, three keys
        txns = ks._single([3, 4, 3, 5, 4])
    elif name.startswith("edge"):    # one key with n signatures among as many keys seen once, interleaved
        n = int(name[4:])
        txns = ks._single([0 if t % 2 == 0 else 6000 + t for t in range(2 * n)])
    elif name == "alternate":        # key 0 and key 1 alternating, 40 signatures each
        txns = ks._single([t & 1 for t in range(80)])
    elif name == "eight_c":          # 8 keys x 4 signatures, none of them in eight_a or eight_b
        txns = ks._single([40 + t % 8 for t in range(32)])
    elif name == "one_each":         # one signature of each of the four keys test_claims_never_evict_a_pin pins
        txns = ks._single([0, 1, 20, 21])
    elif name == "sampled":          # 300 signatures, every key distinct but key 0's: five in the first 256 lanes, five behind
        at = (10, 20, 30, 40, 50, 260, 265, 270, 275, 280)
        txns = ks._single([0 if t in at else 3000 + t for t in range(300)])
    else:
        return kc._batch(name)
    return ks._pack(txns)


OWN = ("fifteen", "one", "five", "alternate", "eight_c", "one_each", "sampled") + tuple("edge%d" % n for n in EDGES)


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    if name not in OWN:
        return kc._want(name, sem)
    p, d, n = _batch(name)
    return ks._oracle().verify_txns(p, d, n, sem=sem, threads=ks.THREADS)


@functools.lru_cache(maxsize=None)
def _comp(name):
    """{key: (signatures in well-formed transactions, those of them with S < l)} of a batch"""
    p, d, n = _batch(name)
    cnt, walk = collections.Counter(), collections.Counter()
    for t in range(len(d)):
        c, sz = int(d["sig_cnt"][t]), int(d["payload_sz"][t])
        if (c == 0 or c > 16 or int(d["signature_off"][t]) + 64 * c > sz or int(d["acct_addr_off"][t]) + 32 * c > sz
                or int(d["message_off"][t]) > sz):
            continue
        for j in range(c):
            at = int(d["payload_off"][t]) + int(d["acct_addr_off"][t]) + 32 * j
            sg = int(d["payload_off"][t]) + int(d["signature_off"][t]) + 64 * j
            key = p[at: at + 32].tobytes()
            cnt[key] += 1
            walk[key] += int.from_bytes(p[sg + 32: sg + 64].tobytes(), "little") < L
    return {k: (cnt[k], walk[k]) for k in cnt}


def _expect(name, pins):
    """((pinned keys in the batch, their signatures), the signatures of those that reach the walk): a pinned key's
    signatures in well-formed transactions are fixed-base; one walks when S < l and the key has tables (every key
    here but tests/test_gpu_key_split.py's four edge keys)."""
    comp, bad = _comp(name), set(ks._edge_keys())
    have = [k for k in dict.fromkeys(pins) if k in comp]
    return (len(have), sum(comp[k][0] for k in have)), sum(comp[k][1] for k in have if k not in bad)


def _go(eng, name, sem, what=None):
    p, d, _ = _batch(name)
    got = eng.verify_txns_host(p, d)
    assert np.isin(got[1], (0, -1, -2, -3)).all(), np.unique(got[1])        # nothing left in flight (FD_PEND_*)
    ks._check(got, _want(name, sem), (name, what))
    return got[1]


def _pinned_batch(eng, name, sem, pins, what=None):
    """Runs a batch whose only fixed-base keys are pinned ones: the counts are the fixture's"""
    s = _go(eng, name, sem, what)
    keys_sigs, walkers = _expect(name, pins)
    assert eng.pinned_count() == keys_sigs, (name, what, eng.pinned_count(), keys_sigs)
    assert eng.fixed_count() == keys_sigs, (name, what, eng.fixed_count())
    assert eng.ffull_count() == (keys_sigs[0], walkers), (name, what, eng.ffull_count(), walkers)
    assert eng.fcache_count() == (0, 0), (name, what, eng.fcache_count())
    return s


def _status(enc):
    """rc of the oracle's decode, and whether the point has small order ([8]P = O); None where it does not decode"""
    rc = ks._oracle().point_decode(enc, 0)[0]
    if rc == 1:
        return rc, None
    return rc, int(torsion._eq(torsion._mul(8, torsion._point_from_enc(enc)), torsion.IDENT))


def _check_status(st, keys):
    assert len(st) == len(keys)
    for b, k in zip(st, keys):
        rc, small = _status(k)
        assert int(b) & 3 == rc, (k.hex(), int(b), rc)
        if small is not None:
            assert int(b) >> 2 == small, (k.hex(), int(b), small)


# ---- the fixtures (CPU) ------------------------------------------------------------------------------------

def test_fixtures():
    """(CPU only, but they are this module's.)  Which keys a case pins, how many signatures each has in well-formed
    transactions and how many of those have S < l: the counts the GPU cases expect are these"""
    p16, p20 = [_pub(i) for i in range(16)], [_pub(i) for i in range(20)]
    assert _expect("fifteen", p16) == ((16, 240), 240) and _expect("fifteen", p20) == ((20, 300), 300)
    assert _expect("fifteen", [_pub(0), _pub(1)]) == ((2, 30), 30) and _expect("fifteen", [_pub(1), _pub(2)]) == ((2, 30), 30)
    assert len(_comp("fifteen")) == 20 and set(_comp("fifteen").values()) == {(15, 15)}
    assert _expect("one", [_pub(3)]) == ((1, 1), 1) and _expect("five", [_pub(3), _pub(4), _pub(5)]) == ((3, 5), 5)
    for n in EDGES:
        assert _expect("edge%d" % n, [_pub(0)]) == ((1, n), n) and len(_comp("edge%d" % n)) == n + 1
    assert _expect("alternate", [_pub(0)]) == ((1, 40), 40) and _comp("alternate")[_pub(1)] == (40, 40)
    edge = ks._edge_keys()
    assert _expect("bad_keys", edge + [_pub(1)]) == ((5, 650), 130)
    assert [_status(k) for k in edge] == [(1, None), (2, 1), (0, 1), (0, 1)] and _status(_pub(1)) == (0, 0)
    tk = list(_comp("torsion"))
    assert len(tk) == 4 and _expect("torsion", tk) == ((4, 40), 40) and all(_status(k) == (0, 0) for k in tk)
    assert _expect("bad_sigs", [_pub(7)]) == ((1, 176), 160)
    assert _expect("malformed", [_pub(0), _pub(1)]) == ((2, 320), 320)
    assert _expect("multi", [_pub(i) for i in range(6)]) == ((6, 300), 300) and len(_comp("multi")) == 156
    assert _expect("one_each", [_pub(i) for i in (0, 1, 20, 21)]) == ((4, 4), 4)
    for name in ("eight_a", "eight_b"):
        assert _expect(name, [_pub(i) for i in (0, 1, 20, 21)]) == ((2, 8), 8) and len(_comp(name)) == 8
    assert _expect("eight_c", [_pub(i) for i in (0, 1, 20, 21)]) == ((0, 0), 0) and len(_comp("eight_c")) == 8
    assert _expect("ten_keys", [_pub(i) for i in (0, 1, 20, 21)]) == ((2, 8), 8) and len(_comp("ten_keys")) == 10
    assert _expect("key0_x3", [_pub(0)]) == ((1, 3), 3) and _comp("one_key") == {_pub(0): (300, 300)}
    assert _expect("sampled", [_pub(0)]) == ((1, 10), 10) and len(_comp("sampled")) == 291
    assert len(_comp("no_repeat")) == 300


# ---- 1, 12: fifteen each; replacing and clearing the set ---------------------------------------------------

@_once
def _fifteen_each(sem, fold):
    pins = [_pub(i) for i in range(16)]
    eng = _engine([_batch("fifteen")], sem, fold=fold)
    never = _engine([_batch("fifteen")], sem, fold=fold)
    try:
        assert eng.pin_cap() == 24 and never.pin_cap() == 24
        _check_status(eng.set_pinned_keys(pins), pins)
        s = _pinned_batch(eng, "fifteen", sem, pins)
        assert eng.hot_count() == (20, 300)                      # keys 16..19 are hot, not fixed-base
        s0 = _go(never, "fifteen", sem, "never pinned")
        assert never.fixed_count() == (0, 0) and never.pinned_count() == (0, 0) and never.ffull_count() == (0, 0)
        assert never.hot_count() == (20, 300)
        np.testing.assert_array_equal(s, s0)
    finally:
        eng.close()
        never.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_fifteen_each(sem, fold):
    """Fifteen signatures a key: 16 pinned keys' 240 signatures walk without doublings; on a context that never
    pinned, none is fixed-base"""
    _fifteen_each(sem, fold)


@_once
def _replace_and_clear(sem, fold):
    eng = _engine([_batch("fifteen")], sem, fold=fold)
    try:
        for pins in ([_pub(0), _pub(1)], [_pub(1), _pub(2)]):
            eng.set_pinned_keys(pins)
            _pinned_batch(eng, "fifteen", sem, pins, "pinned %d" % len(pins))      # (2, 30): the other key is not
        assert len(eng.set_pinned_keys([])) == 0
        _go(eng, "fifteen", sem, "unpinned")
        assert eng.fixed_count() == (0, 0) and eng.pinned_count() == (0, 0) and eng.ffull_count() == (0, 0)
        assert eng.hot_count() == (20, 300) and eng.fcache_count() == (0, 0)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_replacing_and_clearing_the_set(sem, fold):
    _replace_and_clear(sem, fold)


# ---- 2, 3: batches below fb_min signatures in all; wave and block edges ------------------------------------

@_once
def _tiny_batches(sem, fold):
    pins = [_pub(3), _pub(4), _pub(5)]
    eng = _engine([_batch("five")], sem, fold=fold)
    try:
        eng.set_pinned_keys(pins)
        for name in ("one", "five", "one"):
            assert (_pinned_batch(eng, name, sem, pins) == 0).all()
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_batches_below_fb_min_in_all(sem, fold):
    """A batch of 1 and of 5 signatures: the fixed-base blocks and the R-check chain run, and the codes are final"""
    _tiny_batches(sem, fold)


@_once
def _edges(n, sem, fold):
    eng = _engine([_batch("edge%d" % n)], sem, fold=fold)
    try:
        eng.set_pinned_keys([_pub(0)])
        assert (_pinned_batch(eng, "edge%d" % n, sem, [_pub(0)]) == 0).all()
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("n", EDGES)
def test_wave_and_block_edges(n, sem, fold):
    _edges(n, sem, fold)


# ---- 4: a wave shared with a fresh claim -------------------------------------------------------------------

@_once
def _shared_wave(sem, fold):
    eng = _engine([_batch("alternate")], sem, fixed=TESTS, fold=fold, max_sig=None)
    try:
        eng.set_pinned_keys([_pub(0)])
        s = _go(eng, "alternate", sem, "key 1 claims")
        assert (s == 0).all() and eng.pinned_count() == (1, 40) and eng.fixed_count() == (2, 80)
        assert eng.fcache_count() == (0, 1) and eng.ffull_count() == (1, 0)       # every wave holds key 1: 8 tables
        s = _go(eng, "alternate", sem, "key 1 promoted")
        assert (s == 0).all() and eng.pinned_count() == (1, 40) and eng.fixed_count() == (2, 80)
        assert eng.fcache_count() == (1, 0) and eng.ffull_count() == (2, 80)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_a_wave_shared_with_a_fresh_claim(sem, fold):
    """key_fixed = 2, key_full = 0: a pinned key alternates with a key that claims a slot in this batch, so every wave
    walks with doublings from the tables every slot has; the same batch again, and all of it walks full"""
    _shared_wave(sem, fold)


# ---- 5, 6, 7, 8: keys without tables, torsion, bad signatures, malformed and multi-signer transactions ------

@_once
def _keys_without_tables(sem, fold):
    pins = ks._edge_keys() + [_pub(1)]
    eng = _engine([_batch("bad_keys")], sem, fold=fold)
    try:
        _check_status(eng.set_pinned_keys(pins), pins)
        s1 = _pinned_batch(eng, "bad_keys", sem, pins, 1)
        s2 = _pinned_batch(eng, "bad_keys", sem, pins, 2)
        np.testing.assert_array_equal(s1, s2)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_keys_without_tables(sem, fold):
    """An undecodable key, x = 0 with the sign bit and keys of order 4 and 8 are pinned too: no tables, the status
    replayed, batch after batch"""
    _keys_without_tables(sem, fold)


@_once
def _named(name, pin_ids, sem, fold):
    pins = list(_comp(name)) if pin_ids is None else [_pub(i) for i in pin_ids]
    eng = _engine([_batch(name)], sem, fold=fold)
    try:
        _check_status(eng.set_pinned_keys(pins), pins)
        _pinned_batch(eng, name, sem, pins)
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("name,pin_ids", [("torsion", None), ("bad_sigs", (7,)), ("malformed", (0, 1)),
                                          ("multi", (0, 1, 2, 3, 4, 5))])
@gpu
def test_named_batches_under_pinned_keys(name, pin_ids, sem, fold):
    """The four torsion kinds; S changed, S >= l, another message and corrupted R under a pinned key; malformed
    transactions among pinned signatures (their lanes load no key); three signers, pinned and cold in every order"""
    _named(name, pin_ids, sem, fold)


# ---- 9: claims never evict a pin ---------------------------------------------------------------------------

FOUR = (0, 1, 20, 21)


@_once
def _claims_never_evict(cache, sem, fold):
    exact = cache == ON
    names = ["eight_c" if exact else "ten_keys", "eight_a", "eight_b", "eight_a", "eight_b"]
    pins = [_pub(i) for i in FOUR]
    eng = _engine([_batch(n) for n in names], sem, fixed=TESTS, cache=cache, fold=fold, max_sig=32 if exact else None)
    try:
        assert eng.pin_cap() == 6
        eng.set_pinned_keys(pins)
        for run, name in enumerate(names):
            _go(eng, name, sem, run)
            hits, builds = eng.fcache_count()
            assert hits + builds <= 4, (name, run, hits, builds)
            pk = eng.pinned_count()
            if exact:                # 8 keys at the bound: the pinned ones found, four of the others in the four free slots
                assert pk == _expect(name, pins)[0] and hits + builds == 4
                assert eng.fixed_count()[0] == pk[0] + 4
            else:
                assert pk[0] <= _expect(name, pins)[0][0] and pk[1] <= _expect(name, pins)[0][1]
        s = _go(eng, "one_each", sem, "after the claims")
        assert (s == 0).all()
        if exact:
            assert eng.pinned_count() == (4, 4) and eng.ffull_count() == (4, 4) and eng.fcache_count() == (0, 0)
        else:
            assert eng.pinned_count()[0] <= 4 and eng.fcache_count() == (0, 0)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("how,cache", [("exact", ON), ("tiny", TESTS)])
def test_claims_never_evict_a_pin(how, cache, sem, fold):
    """8 slots, 4 of them pinned: batches with more keys at the bound than free slots claim the other four over and
    over, and a signature of each pinned key still walks full afterwards.  With the two-probe index of key_cache = 2 a
    pinned slot may find no place in a batch's index, so there the codes and the bounds are checked."""
    _claims_never_evict(cache, sem, fold)


# ---- 10, 11: key_cache = 1; pinning a resident key ---------------------------------------------------------

@_once
def _cache_off(sem, fold):
    pins = [_pub(i) for i in range(16)]
    eng = _engine([_batch("fifteen")], sem, cache=OFF, fold=fold)
    try:
        eng.set_pinned_keys(pins)
        for run in range(2):
            _pinned_batch(eng, "fifteen", sem, pins, run)        # (fcache_count: no build)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_key_cache_off_keeps_the_pins(sem, fold):
    """key_cache = 1 empties every slot ahead of each batch; the pins stand"""
    _cache_off(sem, fold)


@_once
def _pin_a_resident_key(sem, fold):
    eng = _engine([_batch("one_key"), _batch("key0_x3")], sem, fold=fold)
    try:
        _go(eng, "one_key", sem, "fixed-base by itself")
        assert eng.fixed_count() == (1, 300) and eng.fcache_count() == (0, 1) and eng.pinned_count() == (0, 0)
        eng.set_pinned_keys([_pub(0)])
        _pinned_batch(eng, "key0_x3", sem, [_pub(0)])            # (1, 3), builds 0
        _go(eng, "one_key", sem, "pinned")
        assert eng.pinned_count() == (1, 300) and eng.fixed_count() == (1, 300) and eng.fcache_count() == (0, 0)
        assert eng.ffull_count() == (1, 300)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_pinning_a_resident_key(sem, fold):
    _pin_a_resident_key(sem, fold)


# ---- 13: a batch the de-duplication only sampled -----------------------------------------------------------

@_once
def _sampled(sem, fold):
    eng = _engine([_batch("no_repeat"), _batch("sampled")], sem, fold=fold)
    try:
        eng.set_pinned_keys([_pub(0)])
        _go(eng, "no_repeat", sem)
        assert eng.key_count() == 300 and eng.pinned_count() == (0, 0)
        s = _go(eng, "sampled", sem, "B")
        # sampled: the first 256 lanes look their keys up (252 keys), each of the 44 behind them is its own representative
        assert eng.key_count() == 296
        assert eng.pinned_count() == (6, 10) and eng.ffull_count()[1] == 10 and eng.fixed_count() == (6, 10)
        assert (s == 0).all()
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem,fold", COMBOS)
def test_a_sampled_batch(sem, fold):
    """After an all-distinct batch the next one is only sampled and counts nothing; its ten signatures of a pinned
    key, five inside the sample and five behind it, are still found and walk full"""
    _sampled(sem, fold)


# ---- 14: refusals ------------------------------------------------------------------------------------------

def _refused(eng, keys):
    with pytest.raises(RuntimeError) as e:
        eng.set_pinned_keys(keys)
    return e.value.args[1]


@_once
def _refusals():
    pins = [_pub(i) for i in range(16)]
    eng = _engine([_batch("fifteen")])
    try:
        eng.set_pinned_keys(pins)
        assert _refused(eng, [_pub(100 + i) for i in range(eng.pin_cap() + 1)]) == -1
        _pinned_batch(eng, "fifteen", 0, pins, "the earlier set still serves")
        # a duplicate is pinned once, and both entries get the status
        edge = ks._edge_keys()
        dup = [_pub(0), edge[0], _pub(0), edge[3], edge[0]]
        _check_status(eng.set_pinned_keys(dup), dup)
        _pinned_batch(eng, "fifteen", 0, dup, "duplicates")      # (1, 15): key 0 once
        # -2 while an async submission is filling
        m = ks._msg(0)
        sig, pub = ks._sign(0, m)
        assert eng.submit(sig + pub + m, 0, 64, 96, 1, 7) == 0
        assert _refused(eng, pins) == -2
        eng.flush()
        tags, codes = eng.poll(blocking=True)
        assert list(tags) == [7] and list(codes) == [0]
        _pinned_batch(eng, "fifteen", 0, dup, "after the refusal")
    finally:
        eng.close()
    for o in (dict(half=0), dict(fixed=OFF), dict(half_force_slow=3)):
        eng = _engine([_batch("fifteen")], **o)
        try:
            assert eng.pin_cap() == 0 and _refused(eng, [_pub(0)]) == -1
            assert len(eng.set_pinned_keys([])) == 0
            _go(eng, "fifteen", 0, o)
            assert eng.pinned_count() == (0, 0)
        finally:
            eng.close()


@gpu
def test_refusals():
    _refusals()


# ---- 15: the latency path ignores pins ---------------------------------------------------------------------

@_once
def _latency(sem):
    pins = [_pub(i) for i in range(16)]
    eng = _engine([_batch("fifteen")], sem, small_batch_max=-1)
    try:
        eng.set_pinned_keys(pins)
        _go(eng, "fifteen", sem, "latency")
        assert eng.pinned_count() == (0, 0) and eng.fixed_count() == (0, 0) and eng.key_count() == 0
        p, d, _ = _batch("fifteen")
        for t in range(len(d)):
            o, z = int(d["payload_off"][t]), int(d["payload_sz"][t])
            assert eng.submit(p[o:o + z].tobytes(), int(d["signature_off"][t]), int(d["acct_addr_off"][t]),
                              int(d["message_off"][t]), int(d["sig_cnt"][t]), t) == 0
        eng.flush()
        fb = eng.front_batch()
        assert fb is not None and fb[0] == len(d) and fb[2] > 0, fb         # lanes per signature: a latency path
        got = 0
        while got < len(d):
            tags, codes = eng.poll(blocking=True)
            assert (codes == 0).all()
            got += len(tags)
        assert eng.pinned_count() == (0, 0)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("sem", [0, 1])
def test_the_latency_path_ignores_pins(sem):
    _latency(sem)
