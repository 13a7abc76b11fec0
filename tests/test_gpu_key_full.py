"""GPU: a fixed-base key that the context's cache has seen in an earlier batch is promoted: its slot gets a table for
every byte of k, and a wave whose lanes all have such a key walks without doublings (the promotion in
fd_keyclass_kernel, the P_j chains behind fd_keyclaim_kernel's claims, fd_ftab_kernel's work items, the body
dsmf_full of fd_dsmh_kernel).

Every case runs small batches forced onto the throughput path (small_batch_max = 0, key_fixed = 2: fixed-base from 4
signatures, key_split = 2), in both result-code semantics and through the unfolded and the carry-folded kernels.
The transaction and per-signature codes always equal the CPU oracle's, and the device's own counts (ffull_count: the
fixed-base keys whose slot was full at the walk, and the signatures that walked without doublings) are the
batch's, so the body cannot be silently off.  The batch helpers are tests/test_gpu_key_split.py's,
tests/test_gpu_key_fixed.py's and tests/test_gpu_key_cache.py's.

Two of the cases ask for 8 slots, so that a batch promotes at most pmax = 2.  With fdgpu_debug_opts_t.key_cache = 2
the 8 slots come with an 8-word index of two probes, which by design cannot hold every resident: a
resident it drops is a miss, claims a slot and starts again with 8 tables, so the count of full slots is then
bounded but not exact.  Those cases therefore run on two contexts: one of max_sig = 32, which has the same 8 slots
(32 / 4) and pmax = 2 behind the ordinary index, where the counts are exact, and the key_cache = 2 one, where the
codes and the bounds are checked.
"""
import collections
import functools
import hashlib

import numpy as np
import pytest

from tests import test_gpu_key_cache as kc
from tests import test_gpu_key_fixed as kf
from tests import test_gpu_key_split as ks

pytestmark = pytest.mark.gpu

ON, OFF, TESTS = 0, 1, 2
L = ks.L
COMBOS = [(0, False), (0, True), (1, False), (1, True)]      # (semantics, carry-folded kernels)


def _once(f):
    """The suite repeats every GPU test per engine path (tests/conftest.py); this module chooses its engine options
    itself, so a scenario runs on the GPU once and the repeats only find that it passed."""
    return functools.lru_cache(maxsize=None)(f)


def _engine(batches, sem=0, full=ON, cache=ON, fold=False, max_sig=None):
    import firedancer_amd as fa
    from firedancer_amd import engine
    fa.load_library()
    engine.debug_set_opts(half=1, small_batch_max=0, key_fixed=TESTS, key_split=2, key_cache=cache, key_full=full,
                          nofold_max=0 if fold else -1)
    try:
        return fa.Engine(device=0, max_txn=max(len(b[1]) for b in batches),
                         max_sig=max_sig or max(b[2] for b in batches),
                         max_payload=max(b[0].nbytes for b in batches), semantics=sem)
    finally:
        engine.debug_reset_opts()


DIGIT_MSG0 = 100000                  # the digit-coverage batch signs ks._msg( DIGIT_MSG0 + t ): chosen on the CPU, see
                                     # test_digit_coverage_fixture


@functools.lru_cache(maxsize=None)
def _batch(name):
    if name == "digits":             # 1 key x 2,048 signatures
        txns = [(ks._msg(DIGIT_MSG0 + t), [ks._sign(0, ks._msg(DIGIT_MSG0 + t))]) for t in range(2048)]
    elif name == "key0_x300":
        txns = ks._single([0] * 300)
    elif name == "mixed":            # key 0 and key 1 alternating, 150 each: every wave holds both
        txns = ks._single([t & 1 for t in range(300)])
    else:
        return kc._batch(name)
    return ks._pack(txns)


OWN = ("digits", "key0_x300", "mixed")


@functools.lru_cache(maxsize=None)
def _want(name, sem):
    if name not in OWN:
        return kc._want(name, sem)
    p, d, n = _batch(name)
    return ks._oracle().verify_txns(p, d, n, sem=sem, threads=ks.THREADS)


@functools.lru_cache(maxsize=None)
def _walkers(name, bound=4):
    """(keys, signatures) of the batch's fixed-base keys that have tables, and of their signatures that reach the
    walk: the key has at least bound signatures in well-formed transactions, decodes and is not of small order
    (every key of these batches but tests/test_gpu_key_split.py's four edge keys), and S < l.  What R is does not
    matter: a fixed-base signature's R is compared after the walk."""
    p, d, n = _batch(name)
    bad = set(ks._edge_keys())
    cnt, walk = collections.Counter(), collections.Counter()
    for t in range(len(d)):
        c, sz = int(d["sig_cnt"][t]), int(d["payload_sz"][t])
        if (int(d["signature_off"][t]) + 64 * c > sz or int(d["acct_addr_off"][t]) + 32 * c > sz
                or int(d["message_off"][t]) > sz):
            continue
        for j in range(c):
            at = int(d["payload_off"][t]) + int(d["acct_addr_off"][t]) + 32 * j
            sg = int(d["payload_off"][t]) + int(d["signature_off"][t]) + 64 * j
            key = p[at: at + 32].tobytes()
            cnt[key] += 1
            walk[key] += int.from_bytes(p[sg + 32: sg + 64].tobytes(), "little") < L
    keys = [k for k, c in cnt.items() if c >= bound and k not in bad]
    return len(keys), sum(walk[k] for k in keys)


def _go(eng, name, sem, what=None):
    """Runs the batch, checks its codes, returns (signature codes, ffull_count)"""
    p, d, _ = _batch(name)
    got = eng.verify_txns_host(p, d)
    assert np.isin(got[1], (0, -1, -2, -3)).all(), np.unique(got[1])        # nothing left in flight (FD_PEND_*)
    ks._check(got, _want(name, sem), (name, what))
    return got[1], eng.ffull_count()


# ---- key_full = 2: a claim fills its slot at once -------------------------------------------------------

FRESH = ["one_key", "counts", "interleaved", "multi", "edge255", "edge256", "edge257", "bad_sigs", "bad_keys",
         "torsion", "hs_top", "malformed", "cap"]


@_once
def _fresh(name, sem, fold):
    eng = _engine([_batch(name)], sem, full=TESTS, fold=fold)
    try:
        _, (keys, sigs) = _go(eng, name, sem, "key_full=2")
        if name == "cap":            # FD_FB_CAP + 4 keys of 4 valid signatures: which FD_FB_CAP get a slot is the device's choice
            assert eng.fixed_count() == (kf.FB_CAP, 4 * kf.FB_CAP) and sigs == 4 * kf.FB_CAP, (keys, sigs)
        else:
            assert sigs == _walkers(name)[1], (name, sem, fold, keys, sigs, _walkers(name))
            assert keys == eng.fixed_count()[0]                  # (every claimed slot is marked full, tables or not)
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("name", FRESH)
def test_fresh_context_walks_without_doublings(name, sem, fold):
    _fresh(name, sem, fold)


def test_cases_have_teeth():
    """(CPU only, but they are this module's.)  The batches hold signatures that walk, and the ones with bad S, bad
    keys and malformed transactions hold some that do not"""
    assert _walkers("one_key") == (1, 300) and _walkers("counts") == (8, 585)
    assert _walkers("bad_sigs") == (1, 160) and _walkers("bad_keys") == (1, 130)
    assert _walkers("malformed") == kf._repeated("malformed", 4) and _walkers("malformed")[0] == 2
    assert _walkers("torsion") == (4, 40) and _walkers("multi")[0] == 6
    assert _walkers("digits") == (1, 2048) and _walkers("mixed") == (2, 300)


# ---- key_full = 0: a key is promoted in the first batch that finds it resident -------------------------

@_once
def _three_times(name, sem, fold):
    eng = _engine([_batch(name)], sem, fold=fold)
    try:
        n = kf._repeated(name, 4)[0]
        s1, ff = _go(eng, name, sem, 1)
        assert ff == (0, 0) and eng.fcache_count() == (0, n)
        s2, ff = _go(eng, name, sem, 2)
        assert eng.fcache_count() == (n, 0)
        assert ff == _walkers(name), (name, ff)                  # the hits that have tables; every walking signature
        s3, ff = _go(eng, name, sem, 3)
        assert eng.fcache_count() == (n, 0) and ff == _walkers(name)
        np.testing.assert_array_equal(s1, s2)
        np.testing.assert_array_equal(s1, s3)
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("name", ["counts", "interleaved", "multi", "bad_sigs", "malformed"])
def test_same_batch_three_times(name, sem, fold):
    """Run 1 claims and walks with doublings; run 2 finds every key resident, promotes it and walks without; run 3
    builds nothing and promotes nothing"""
    _three_times(name, sem, fold)


def _k_digits(sig, pub, msg):
    k = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % L
    d, carry = [], 0
    for j in range(32):              # fd_fb_recode
        v = ((k >> (8 * j)) & 255) + carry
        carry = (v + 128) >> 8
        d.append(v - (carry << 8))
    return d


@_once
def _digits_seen():
    seen = [set() for _ in range(32)]
    pub = ks._key(0)[0]
    for t in range(2048):
        m = ks._msg(DIGIT_MSG0 + t)
        for j, x in enumerate(_k_digits(ks._sign(0, m)[0], pub, m)):
            seen[j].add(x)
    return seen


def test_digit_coverage_fixture():
    """(CPU only.)  Every table j meets a digit 0, a -128 and a +127 in the batch: the identity entry, the last entry
    negated and the last but one.  Table 31 is the exception no batch can fill: k < l < 2^253 bounds its digit by
    0x0f plus a carry, so it must meet 0 and 16, the two ends of what it can hold."""
    seen = _digits_seen()
    for j in range(31):
        assert {0, -128, 127} <= seen[j], j
    assert {0, 16} <= seen[31] and max(seen[31]) == 16 and min(seen[31]) == 0


@_once
def _digit_coverage(sem, fold):
    eng = _engine([_batch("digits")], sem, fold=fold)
    try:
        s, ff = _go(eng, "digits", sem, 1)
        assert ff == (0, 0) and (s == 0).all()
        s, ff = _go(eng, "digits", sem, 2)
        assert ff == (1, 2048) and (s == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
def test_digit_coverage(sem, fold):
    """One key x 2,048 valid signatures whose digits reach every table's ends (test_digit_coverage_fixture), with
    doublings and then without: every signature verifies both ways"""
    _digit_coverage(sem, fold)


@_once
def _mixed_wave(sem, fold):
    eng = _engine([_batch("key0_x300"), _batch("mixed")], sem, fold=fold)
    try:
        assert _go(eng, "key0_x300", sem, 1)[1] == (0, 0)
        assert _go(eng, "key0_x300", sem, 2)[1] == (1, 300)
        s, ff = _go(eng, "mixed", sem, "key 1 is new")
        assert ff == (1, 0) and (s == 0).all()                   # key 0 is full, and no wave is of key 0 alone
        s, ff = _go(eng, "mixed", sem, "key 1 promoted")
        assert ff == (2, 300) and (s == 0).all()
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
def test_mixed_wave(sem, fold):
    """A wave that holds one signature of a key not yet promoted walks with doublings, all of it"""
    _mixed_wave(sem, fold)


# ---- 8 slots: pmax = 2 -----------------------------------------------------------------------------------

EIGHT = [("exact", ON, 32), ("tiny", TESTS, None)]            # (see the module's docstring)


@_once
def _promotion_cap(cache, max_sig, sem, fold):
    eng = _engine([_batch("eight_a")], sem, cache=cache, fold=fold, max_sig=max_sig)
    try:
        first = None
        for run in range(6):
            s, (keys, sigs) = _go(eng, "eight_a", sem, run)
            assert (s == 0).all()
            first = s if first is None else first
            np.testing.assert_array_equal(first, s)
            if cache == ON:
                assert keys == min(8, 2 * run), (run, keys)      # 0, 2, 4, 6, 8, 8
                assert sigs == (32 if keys == 8 else 0)          # (the 32 signatures are one wave)
            else:
                assert keys <= min(8, 2 * run) and keys <= eng.fcache_count()[0] and sigs in (0, 32)
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("how,cache,max_sig", EIGHT)
def test_promotion_cap(how, cache, max_sig, sem, fold):
    """8 keys resident in 8 slots: a batch promotes two of them and leaves the others for the batches after"""
    _promotion_cap(cache, max_sig, sem, fold)


@_once
def _eviction(cache, max_sig, sem, fold):
    eng = _engine([_batch("eight_a"), _batch("eight_b")], sem, cache=cache, fold=fold, max_sig=max_sig)
    try:
        _go(eng, "eight_a", sem, 1)
        _, ff = _go(eng, "eight_a", sem, 2)
        assert ff[0] == 2 if cache == ON else ff[0] <= 2
        s, ff = _go(eng, "eight_b", sem, "evicts")               # a stale full word would walk another key's tables
        assert (s == 0).all() and ff == (0, 0)
        s, ff = _go(eng, "eight_b", sem, "promoted")
        assert (s == 0).all() and (ff == (2, 0) if cache == ON else ff[0] <= 2)
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("how,cache,max_sig", EIGHT)
def test_eviction_clears_full(how, cache, max_sig, sem, fold):
    _eviction(cache, max_sig, sem, fold)


# ---- keys without tables, and the option off -------------------------------------------------------------

@_once
def _keys_without_tables(sem, fold):
    eng = _engine([_batch("bad_keys")], sem, fold=fold)
    try:
        s1, ff = _go(eng, "bad_keys", sem, 1)
        assert ff == (0, 0) and eng.fcache_count() == (0, 5)
        for run in (2, 3):
            s, ff = _go(eng, "bad_keys", sem, run)
            assert eng.fcache_count() == (5, 0)
            assert ff[0] == 1, ff                                # key 1 alone: the four others have nothing to promote
            np.testing.assert_array_equal(s1, s)
    finally:
        eng.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
def test_keys_without_tables_are_never_promoted(sem, fold):
    """An undecodable key, x = 0 with the sign bit and two small-order keys beside a good one, 130 signatures each:
    their slots replay the status and the codes, and stay as they are"""
    _keys_without_tables(sem, fold)


@_once
def _option_off(name, sem, fold):
    eng = _engine([_batch(name)], sem, full=OFF, fold=fold)
    on = _engine([_batch(name)], sem, fold=fold)
    try:
        for run in range(3):
            s, ff = _go(eng, name, sem, run)
            assert ff == (0, 0)
            s_on, _ = _go(on, name, sem, run)
            np.testing.assert_array_equal(s, s_on)
        assert eng.fcache_count() == (kf._repeated(name, 4)[0], 0)
    finally:
        eng.close()
        on.close()


@pytest.mark.parametrize("sem,fold", COMBOS)
@pytest.mark.parametrize("name", ["counts", "bad_sigs"])
def test_key_full_off(name, sem, fold):
    """key_full = 1: nothing is ever promoted, and the codes are those of the option on, batch by batch"""
    _option_off(name, sem, fold)
