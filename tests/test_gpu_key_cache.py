"""GPU: a context keeps the tables of its fixed-base keys from batch to batch (the key cache: the index role of
fd_keydedup_kernel, the look-up of fd_keyclass_kernel, fd_keyclaim_kernel, and fbase_build and fd_ftab_kernel over
the keys claimed in a batch).

Every case runs batches of a few hundred signatures on the throughput path (small_batch_max = 0) of one context,
one after another, with fdgpu_debug_opts_t.key_fixed = 2 (a key is fixed-base from 4 signatures) unless stated, and
checks the transaction and per-signature codes of every batch against the CPU oracle, together with the device's
own counts: the batch's fixed-base keys (fixed_count), and how many of them were found resident and how many
built their tables (fcache_count).  The batch helpers are tests/test_gpu_key_split.py's and
tests/test_gpu_key_fixed.py's.
"""
import collections
import functools

import numpy as np
import pytest

from tests import test_gpu_key_fixed as kf
from tests import test_gpu_key_split as ks

pytestmark = pytest.mark.gpu

ON, OFF, TESTS = 0, 1, 2
FOLDS = [False, True]                # the unfolded walk of small batches and (nofold_max = 0) the large batches' folded one


def _once(f):
    """The suite repeats every GPU test per engine path (tests/conftest.py); this module chooses its engine options
    itself, so a scenario runs on the GPU once and the repeats only find that it passed."""
    return functools.lru_cache(maxsize=None)(f)


def _engine(batches, sem=0, fixed=TESTS, cache=ON, fold=False):
    """A context that holds the largest of batches"""
    import firedancer_amd as fa
    from firedancer_amd import engine
    fa.load_library()
    engine.debug_set_opts(half=1, small_batch_max=0, key_fixed=fixed, key_split=2 if fixed == TESTS else 0,
                          key_cache=cache, nofold_max=0 if fold else -1)
    try:
        return fa.Engine(device=0, max_txn=max(len(b[1]) for b in batches), max_sig=max(b[2] for b in batches),
                         max_payload=max(b[0].nbytes for b in batches), semantics=sem)
    finally:
        engine.debug_reset_opts()


@functools.lru_cache(maxsize=None)
def _flipped_key():
    """Key 0 with one bit changed, such that the encoding still decodes to a point (so it gets tables of its own)"""
    pub = ks._key(0)[0]
    for bit in range(8, 248):
        x = bytearray(pub)
        x[bit >> 3] ^= 1 << (bit & 7)
        if ks._oracle().point_decode(bytes(x), 0)[0] == 0 and ks._oracle().point_decode(bytes(x), 1)[0] == 0:
            return bytes(x)
    raise AssertionError("no decodable neighbour")


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(payload, desc, nsig) of this module's own cases; every other name is tests/test_gpu_key_fixed.py's"""
    if name == "key7":               # 20 valid signatures of the key that fixed's bad_sigs corrupts
        txns = ks._single([7] * 20)
    elif name == "flipped":          # 8 signatures of key 0 filed under its one-bit neighbour: none verifies
        txns = [(m, [(sig, _flipped_key())]) for m, [(sig, _)] in ks._single([0] * 8)]
    elif name == "flipped_and_true": # ... and the same beside 8 valid signatures under key 0 itself
        txns = ks._single([0] * 16)
        txns = [(m, [(sig, _flipped_key() if t % 2 else pub)]) for t, (m, [(sig, pub)]) in enumerate(txns)]
    elif name == "key0_x3":          # below the bound of 4
        txns = ks._single([0, 0, 0] + list(range(9000, 9010)))
    elif name == "key0_x5":
        txns = ks._single([0] * 5 + list(range(9000, 9010)))
    elif name == "ten_keys":         # 10 keys x 4 signatures: two more than the test mode's 8 slots
        txns = ks._single([t % 10 for t in range(40)])
    elif name in ("eight_a", "eight_b"):   # 8 keys x 4 signatures, the two sets disjoint
        txns = ks._single([(0 if name[-1] == "a" else 20) + t % 8 for t in range(32)])
    elif name == "triples":          # 100 keys x 3 signatures: hot (from 2 on), none fixed-base
        txns = ks._single([100 + t % 100 for t in range(300)])
    elif name == "scattered":        # 70 keys x 4 signatures shuffled among 200 keys seen once: 270 representatives
        keys = [t % 70 for t in range(280)] + list(range(8000, 8200))
        np.random.default_rng(17).shuffle(keys)
        txns = ks._single(keys)
    else:
        return kf._batch(name)
    return ks._pack(txns)


OWN = ("key7", "flipped", "flipped_and_true", "key0_x3", "key0_x5", "ten_keys", "eight_a", "eight_b", "scattered", "triples")


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    """The oracle's codes, computed once (tests/test_gpu_key_fixed.py's own for its batches)"""
    if name not in OWN:
        return kf._want(name, sem)
    p, d, n = _batch(name)
    return ks._oracle().verify_txns(p, d, n, sem=sem, threads=ks.THREADS)


@functools.lru_cache(maxsize=None)
def _repeated(name, bound):
    """(keys, signatures) of the batch's keys with >= bound signatures, as tests/test_gpu_key_fixed.py counts them"""
    if name not in OWN:
        return kf._repeated(name, bound)
    p, d, n = _batch(name)                                       # (this module's own: well-formed, one signer each)
    keys = collections.Counter(p[int(o) + int(a): int(o) + int(a) + 32].tobytes()
                               for o, a in zip(d["payload_off"], d["acct_addr_off"]))
    rep = [c for c in keys.values() if c >= bound]
    return len(rep), sum(rep)


def _go(eng, name, sem, what=None):
    """Runs the batch, checks its codes, returns (fixed-base keys, hits, builds)"""
    p, d, _ = _batch(name)
    got = eng.verify_txns_host(p, d)
    assert np.isin(got[1], (0, -1, -2, -3)).all(), np.unique(got[1])        # nothing left in flight (FD_PEND_*)
    ks._check(got, _want(name, sem), (name, what))
    hits, builds = eng.fcache_count()
    keys = eng.fixed_count()[0]
    assert hits + builds == keys, (name, what, keys, hits, builds)
    return keys, hits, builds


@_once
def _twice(name, sem, fold, fixed=TESTS, bound=4, cache=ON):
    eng = _engine([_batch(name)], sem, fixed, cache, fold)
    try:
        n = _repeated(name, bound)[0]
        assert n > 0
        assert _go(eng, name, sem, "build") == (n, 0, n)
        assert _go(eng, name, sem, "hit") == (n, n, 0)
        assert eng.fixed_count() == _repeated(name, bound)
    finally:
        eng.close()


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("sem", [0, 1])
def test_same_batch_twice(sem, fold):
    """The second time every fixed-base key is resident and nothing is built"""
    _twice("counts", sem, fold)


@pytest.mark.parametrize("fold", FOLDS)
def test_same_batch_twice_product_bound(fold):
    """... with the product's bound of 128: one key x 300 signatures"""
    _twice("one_key", 0, fold, fixed=ON, bound=128)


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", ["bad_keys", "torsion"])
def test_keys_without_tables_twice(name, sem, fold):
    """Keys that do not decode, x = 0 with the sign set and small-order keys (one whose code depends on R's decode):
    the slot replays the status, so the hit batch gives the build batch's codes"""
    _twice(name, sem, fold)


@_once
def _bad_signatures_under_a_cached_key(sem, fold):
    eng = _engine([_batch("key7"), _batch("bad_sigs")], sem, fold=fold)
    try:
        assert _go(eng, "key7", sem) == (1, 0, 1)
        assert _go(eng, "bad_sigs", sem) == (1, 1, 0)
    finally:
        eng.close()


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("sem", [0, 1])
def test_bad_signatures_under_a_cached_key(sem, fold):
    """A bad S, another message and a corrupted, non-canonical, undecodable and small-order R, all in a hit batch"""
    _bad_signatures_under_a_cached_key(sem, fold)


@_once
def _a_key_one_bit_from_a_cached_key(sem):
    assert (_want("flipped", sem)[1] != 0).all()
    s = _want("flipped_and_true", sem)[1]
    assert (s[0::2] == 0).all() and (s[1::2] != 0).all()
    eng = _engine([_batch("flipped_and_true")], sem)
    try:
        assert _go(eng, "flipped", sem) == (1, 0, 1)
        assert _go(eng, "flipped_and_true", sem) == (2, 1, 1)
        assert _go(eng, "flipped_and_true", sem) == (2, 2, 0)
    finally:
        eng.close()


@pytest.mark.parametrize("sem", [0, 1])
def test_a_key_one_bit_from_a_cached_key(sem):
    """The neighbour is cached first (with tables: it decodes); key 0 itself then misses, builds, and its valid
    signatures verify -- with the neighbour's tables they would not.  Afterwards both are resident."""
    _a_key_one_bit_from_a_cached_key(sem)


@_once
def _a_cached_key_below_the_bound():
    eng = _engine([_batch("key0_x5")])
    try:
        assert _go(eng, "key0_x5", 0) == (1, 0, 1)
        assert _go(eng, "key0_x3", 0) == (0, 0, 0)
        assert eng.fixed_count() == (0, 0) and eng.hot_count() == (1, 3)
        assert _go(eng, "key0_x5", 0) == (1, 1, 0)
    finally:
        eng.close()


def test_a_cached_key_below_the_bound():
    """With 3 signatures a cached key is hot like any other and its slot is not touched; with 5 it is a hit"""
    _a_cached_key_below_the_bound()


@_once
def _eight_slots_ten_keys():
    eng = _engine([_batch("ten_keys")], cache=TESTS)
    try:
        assert _go(eng, "ten_keys", 0) == (8, 0, 8)
        for k in range(3):
            keys, hits, builds = _go(eng, "ten_keys", 0, k)
            assert keys == 8 and eng.fixed_count() == (8, 32) and eng.hot_count() == (10, 40)
    finally:
        eng.close()


def test_eight_slots_ten_keys():
    """key_cache = 2: exactly 8 of the 10 keys are fixed-base, the other two stay hot.  Repeated, the residents
    the two-probe index holds are hits and claim nothing; a resident it could not hold is a miss like the two
    surplus keys, and the misses take exactly the slots no hit stamped (_go: hits + builds = 8)."""
    _eight_slots_ten_keys()


@_once
def _eight_slots_alternating_batches():
    eng = _engine([_batch("eight_a"), _batch("eight_b")], cache=TESTS)
    try:
        for name in ("eight_a", "eight_b", "eight_a"):
            assert _go(eng, name, 0) == (8, 0, 8)
        keys, hits, builds = _go(eng, "eight_a", 0, "again")
        assert keys == 8
    finally:
        eng.close()


def test_eight_slots_alternating_batches():
    """key_cache = 2, two disjoint sets of 8 keys: each batch evicts the other's"""
    _eight_slots_alternating_batches()


@_once
def _more_keys_than_slots_repeated():
    eng = _engine([_batch("cap")])
    try:
        assert _go(eng, "cap", 0) == (kf.FB_CAP, 0, kf.FB_CAP)
        assert _go(eng, "cap", 0) == (kf.FB_CAP, kf.FB_CAP, 0)
        assert eng.fixed_count() == (kf.FB_CAP, 4 * kf.FB_CAP)
    finally:
        eng.close()


def test_more_keys_than_slots_repeated():
    """FD_FB_CAP + 4 keys at the bound (tests/test_gpu_key_fixed.py's cap): the second time the FD_FB_CAP resident
    ones are stamped before any claim, so nothing is claimed and nothing built"""
    _more_keys_than_slots_repeated()


@pytest.mark.parametrize("fold", FOLDS)
def test_look_ups_and_claims_across_blocks(fold):
    """270 representatives, the 70 at the bound scattered among them: the look-ups and the miss list span two
    blocks, and the 70 claims more than a wave"""
    _twice("scattered", 0, fold)


@_once
def _sampled_and_hot_only_batches_between_two_uses():
    names = ("one_key", "hot_only", "no_repeat", "triples")
    eng = _engine([_batch(n) for n in names])
    try:
        assert _go(eng, "one_key", 0) == (1, 0, 1)
        assert _go(eng, "triples", 0) == (0, 0, 0) and eng.hot_count() == (100, 300)
        assert _go(eng, "hot_only", 0) == (30, 1, 29)           # (30 keys x 10 signatures, key 0 among them)
        assert _go(eng, "no_repeat", 0) == (0, 0, 0)
        assert _go(eng, "one_key", 0, "B") == (0, 0, 0)         # sampled: 7/8 of the batch before were representatives
        assert eng.hot_count() == (0, 0)
        assert _go(eng, "one_key", 0) == (1, 1, 0)
        assert _go(eng, "hot_only", 0) == (30, 30, 0)
    finally:
        eng.close()


def test_sampled_and_hot_only_batches_between_two_uses():
    """Batches without a fixed-base key -- hot keys only, distinct keys, one that the de-duplication only samples
    ("B") -- leave the slots alone, and a batch of other fixed-base keys has room beside them: the key is still
    resident afterwards"""
    _sampled_and_hot_only_batches_between_two_uses()


@pytest.mark.parametrize("sem", [0, 1])
@pytest.mark.parametrize("name", ["malformed", "multi"])
def test_malformed_and_three_signer_transactions(name, sem):
    _twice(name, sem, False)


@_once
def _cache_off_builds_every_time(sem):
    n = _repeated("counts", 4)
    eng = _engine([_batch("counts")], sem, cache=OFF)
    try:
        for k in range(3):
            assert _go(eng, "counts", sem, k) == (n[0], 0, n[0])
            assert eng.fixed_count() == n
    finally:
        eng.close()


@pytest.mark.parametrize("sem", [0, 1])
def test_cache_off_builds_every_time(sem):
    """key_cache = 1: the codes and the counts of the cache on, and every batch builds all its keys"""
    _cache_off_builds_every_time(sem)


@_once
def _a_new_context_starts_empty():
    for k in range(2):
        eng = _engine([_batch("counts")])
        try:
            assert _go(eng, "counts", 0, k)[1] == 0
        finally:
            eng.close()


def test_a_new_context_starts_empty():
    _a_new_context_starts_empty()
